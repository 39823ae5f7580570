"""fp8q.ops.percentile (csrc/fp8q_select.hip) against the host oracle of the contract (tests/percentile_oracle.py): bit for bit,
on both routes -- rows resident in LDS and the three-pass streaming select -- at the shapes where each takes another path."""
import numpy as np
import pytest
import torch

from percentile_oracle import Oracle, assert_bits, exact_pct

pytestmark = pytest.mark.gpu

PCTS = [0.01, 0.1, 1.0, 5.0, 50.0, 0.0, 100.0, 50.5, 63.0, 99.9]       # past the middle: lo > hi, still the contract


def _R():
    import fp8q
    return fp8q.ops.percentile_resident_max_inner()


def _shape(spec):
    """shapes are written with R = the row-resident limit: (C, (a, b)) means inner = a * R + b"""
    C, n = spec
    return (C, n[0] * _R() + n[1]) if isinstance(n, tuple) else (C, n)


RESIDENT = [(7, 1), (5, 2), (6, 3), (64, 147), (48, 300), (33, 576), (3, 4097), (2, (1, 0))]
STREAMING = [(2, (1, 1)), (3, 70001), (1, (1 << 20) + 77), (1025, (2, 3))]
_ids = lambda s: f"{s[0]}x{'R*%d+%d' % s[1] if isinstance(s[1], tuple) else s[1]}"


def _pcts_for(n):
    e = exact_pct(n)
    return PCTS + ([e] if e is not None else [])


def _run(x, pct, per_channel=True, **kw):
    import fp8q
    lo, hi = fp8q.ops.percentile(x, per_channel, pct, **kw)
    assert lo.dtype == torch.float32 and hi.dtype == torch.float32
    assert lo.shape == hi.shape == ((x.shape[0],) if per_channel else (1,))
    return lo.cpu().numpy(), hi.cpu().numpy()


def _check_all(x_np, x_dev, pcts, per_channel=True, what=""):
    orc = Oracle(x_np if per_channel else x_np.reshape(1, -1))
    for pct in pcts:
        lo, hi = _run(x_dev, pct, per_channel)
        wlo, whi = orc.ranges(pct)
        assert_bits(lo, wlo, (what, pct, "lo"))
        assert_bits(hi, whi, (what, pct, "hi"))
    return orc


def _ulp_check(x_np, x_dev, orc, pcts):
    """np.percentile itself, within 2 float32 ulp of max(|a|, |b|): our t and numpy's differ by rounding noise of order
    n * 2^-53, both round b - a to float32, then comes one final rounding to float32"""
    ref = np.percentile(x_np, [p for pct in pcts for p in (pct, 100.0 - pct)], axis=1)
    for i, pct in enumerate(pcts):
        got = _run(x_dev, pct)
        for side, q in ((0, pct / 100.0), (1, (100.0 - pct) / 100.0)):
            a, b, _ = orc.pair(q)
            bound = 2.0 * np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
            err = np.abs(got[side].astype(np.float64) - ref[2 * i + side])
            assert (err <= bound).all(), (pct, side, err.max(), bound.min())


@pytest.mark.parametrize("spec", RESIDENT + STREAMING, ids=_ids)
def test_seeded_normals_every_percentile(spec):
    C, n = _shape(spec)
    x_np = np.random.RandomState(C * 131 + n % 9973).randn(C, n).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    pcts = _pcts_for(n)
    orc = _check_all(x_np, x, pcts, what=(C, n))
    lo, hi = _run(x, 50.0)
    assert_bits(lo, hi, "at 50 lo == hi")
    if n > 2:
        lo, hi = _run(x, 50.5)
        assert (lo > hi).all()
    lo, hi = _run(x, 0.0)
    assert_bits(lo, x_np.min(axis=1), "rank 0")
    assert_bits(hi, x_np.max(axis=1), "rank n - 1")
    lo, hi = _run(x, 100.0)
    assert_bits(lo, x_np.max(axis=1), "rank n - 1")
    assert_bits(hi, x_np.min(axis=1), "rank 0")
    _ulp_check(x_np, x, orc, [0.01, 0.1, 1.0, 5.0, 50.0])


def test_per_tensor_activation_beyond_torch_quantiles_limit():
    """2^24 + 1 elements (67 MB: the nontemporal variant of the streaming route), per tensor"""
    n = (1 << 24) + 1
    x_np = np.random.RandomState(24).randn(n).astype(np.float32)
    x_np[::2] = np.maximum(x_np[::2], 0.0)                     # plenty of +0.0 keys as well
    x = torch.from_numpy(x_np).cuda()
    _check_all(x_np, x, [0.01, 0.1, 1.0, 50.0, 100.0, 63.0, exact_pct(n)], per_channel=False, what="2^24+1")


def _kinds(rng, C, n):
    normals = rng.randn(C, n).astype(np.float32)
    j = np.stack([rng.permutation(n) for _ in range(C)]).astype(np.uint32)
    relu = np.maximum(normals, 0.0)
    relu[(relu == 0) & (rng.rand(C, n) < 0.3)] = -0.0
    infs = normals.copy()
    infs[rng.rand(C, n) < 0.02] = np.inf
    infs[rng.rand(C, n) < 0.02] = -np.inf
    infs[:, 0] = np.inf                                          # (short rows too)
    one_nan = normals.copy()
    one_nan[1 % C, n // 2] = np.nan
    denorm = (rng.randint(1, 0x800000, size=(C, n)).astype(np.uint32)
              | (rng.randint(0, 2, size=(C, n)).astype(np.uint32) << 31)).view(np.float32)
    return {
        "equal": np.full((C, n), 3.25, np.float32),
        "two_values": rng.choice(np.array([-1.5, 2.25], np.float32), size=(C, n)),
        "small_ints": rng.randint(0, 8, size=(C, n)).astype(np.float32),
        "relu_signed_zeros": relu,
        "negatives": -np.abs(normals) - 0.125,
        "last_digit": (np.uint32(0x3F800000) + (j % 1024)).view(np.float32),            # 1 + j 2^-23
        "middle_digit": (np.uint32(0x3F800000) | ((j % 2048) << 10)).view(np.float32),
        "denormals": denorm,
        "infs": infs,
        "one_nan_row": one_nan,
    }


KINDS = ["equal", "two_values", "small_ints", "relu_signed_zeros", "negatives", "last_digit", "middle_digit", "denormals",
         "infs", "one_nan_row"]
KIND_SHAPES = [(48, 300), (3, 4097), (2, (1, 1)), (3, 70001)]        # a wave per row, a workgroup per row, streaming x 2


@pytest.fixture(scope="module")
def kind_data():
    cache = {}

    def get(spec):
        if spec not in cache:
            C, n = _shape(spec)
            cache[spec] = _kinds(np.random.RandomState(n), C, n)
        return cache[spec]
    return get


@pytest.mark.parametrize("spec", KIND_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", KINDS)
def test_data_kinds(kind, spec, kind_data):
    C, n = _shape(spec)
    x_np = kind_data(spec)[kind]
    x = torch.from_numpy(x_np).cuda()
    _check_all(x_np, x, [0.1, 1.0, 5.0, 50.0, 0.0, 100.0, 63.0, exact_pct(n)], what=(kind, C, n))
    if kind == "one_nan_row":
        lo, hi = _run(x, 1.0)
        bad = 1 % C
        assert np.isnan(lo[bad]) and np.isnan(hi[bad])
        assert not np.isnan(np.delete(lo, bad)).any() and not np.isnan(np.delete(hi, bad)).any()


@pytest.mark.parametrize("spec", [(64, 147), (2, (1, 0)), (2, (1, 1))], ids=_ids)
def test_rows_on_a_base_pointer_4_bytes_off_16_byte_alignment(spec):
    C, n = _shape(spec)
    x_np = np.random.RandomState(n + 1).randn(C * n + 1).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()[1:].view(C, n)
    assert x.data_ptr() % 16 == 4
    _check_all(x_np[1:].reshape(C, n), x, _pcts_for(n), what=("unaligned", C, n))


@pytest.mark.parametrize("spec", [(33, 576), (3, 70001)], ids=_ids)
def test_repeatable_out_parameters_and_a_dirty_workspace(spec):
    import fp8q
    ops = fp8q.ops
    C, n = _shape(spec)
    x_np = np.random.RandomState(3).randn(C, n).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    first = _run(x, 1.0)
    second = _run(x, 1.0)
    assert_bits(first[0], second[0])
    assert_bits(first[1], second[1])
    lo = torch.full((C,), 7.0, device="cuda")
    hi = torch.full((C,), 7.0, device="cuda")
    rlo, rhi = ops.percentile(x, True, 1.0, lo=lo, hi=hi)
    assert rlo is lo and rhi is hi
    assert_bits(lo.cpu().numpy(), first[0])
    assert_bits(hi.cpu().numpy(), first[1])
    nbytes = fp8q.lib().fp8q_percentile_workspace_bytes(C, n)
    if nbytes:
        ops._workspace(x.device, nbytes).fill_(0xFF)          # the call clears what it counts into
        dirty = _run(x, 1.0)
        assert_bits(dirty[0], first[0])
        assert_bits(dirty[1], first[1])
        ops._workspace(x.device, nbytes).zero_()
        clean = _run(x, 1.0)
        assert_bits(clean[0], first[0])
        assert_bits(clean[1], first[1])
    with pytest.raises(fp8q.Fp8qError):
        ops.percentile(x.cpu(), True, 1.0)                     # no fallback
    with pytest.raises(fp8q.Fp8qError):
        ops.percentile(x, True, 101.0)
    with pytest.raises(fp8q.Fp8qError):
        ops.percentile(x, True, 1.0, lo=torch.empty(C + 1, device="cuda"), hi=hi)


def test_non_contiguous_input_per_tensor_and_per_channel():
    x_np = np.random.RandomState(8).randn(4, 6, 5, 7).astype(np.float32)
    x = torch.from_numpy(x_np).cuda().contiguous(memory_format=torch.channels_last)
    assert not x.is_contiguous()
    _check_all(x_np.reshape(1, -1), x, [1.0, 50.0], per_channel=False, what="channels_last per tensor")
    lo, hi = _run(x, 5.0)
    wlo, whi = Oracle(x_np.reshape(4, -1)).ranges(5.0)
    assert_bits(lo, wlo)
    assert_bits(hi, whi)


@pytest.mark.parametrize("spec", [(33, 576), (3, 70001)], ids=_ids)
def test_enqueue_only_on_a_side_stream(spec):
    import fp8q
    from test_sign_syncfree import _NoSync
    C, n = _shape(spec)
    x_np = np.random.RandomState(4).randn(C, n).astype(np.float32)
    x = torch.from_numpy(x_np).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fp8q.ops.percentile(x, True, 1.0)                      # the stream's workspace exists now
    side.synchronize()
    with torch.cuda.stream(side):
        with _NoSync():
            lo, hi = fp8q.ops.percentile(x, True, 1.0)
            lo2, hi2 = fp8q.ops.percentile(x, True, 5.0)
    side.synchronize()
    orc = Oracle(x_np)
    for got, want in ((lo, orc.ranges(1.0)[0]), (hi, orc.ranges(1.0)[1]), (lo2, orc.ranges(5.0)[0]), (hi2, orc.ranges(5.0)[1])):
        assert_bits(got.cpu().numpy(), want)
