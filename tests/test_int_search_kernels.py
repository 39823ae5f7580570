"""The uniform quantizers' line search in one pass (fp8q_int_sse_grid_f32 / _f64, ops.int_sse_grid, and
LineSearchEstimator on top of it).

The element-level reference is this repository's own quantizer classes on CPU tensors: the eager torch chain that
tests/test_int_golden.py pins to the reference.  Candidate k is the quantizer after
set_quant_range(0 or -thr[k], thr[k]) with Python floats, exactly what the estimator's candidate loop does."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _quantizer(sym, n_bits, **kw):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    return (SymmetricUniformQuantizer if sym else AsymmetricUniformQuantizer)(n_bits=n_bits, **kw)


def _candidate(sym, n_bits, one_sided, t):
    q = _quantizer(sym, n_bits)
    q.set_quant_range(0.0 if one_sided else -float(t), float(t))
    return q


def _cpu_squares(x, thr, sym, n_bits, one_sided):
    """[n_cand, *x.shape] (x - q_k(x)) ** 2 of the CPU chain, in x's dtype"""
    return torch.stack([(x - _candidate(sym, n_bits, one_sided, t)(x)) ** 2 for t in thr.tolist()])


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# bit-exact elements: inner = 1, every sum is a single square
# ---------------------------------------------------------------------------------------------------------------------
N_ROWS, N_K = 4096, 65


def _thresholds():
    thr = np.float32(0.0371 * np.arange(1, N_K + 1))
    thr[0], thr[1], thr[2] = 1e-9, 3.0e-8, 2.5e4        # below eps (x_max' = eps), just above it, a wide range
    return thr


def _adversarial(dtype, thr, sym, n_bits, one_sided):
    """4096 values: per candidate exact ties (j + 1/2) * scale_k with both neighbours and the values on / just beyond
    both clamp ends, then +-0, +-inf, denormals, 1e30, and normal draws for the rest"""
    np_dt = np.float32 if dtype == torch.float32 else np.float64
    vals = []
    for t in thr.tolist():
        q = _candidate(sym, n_bits, one_sided, t)
        s = float(q.scale)                               # a float32 value
        lo, hi, zp = float(q.int_min), float(q.int_max), float(q.zero_point)
        js = [0, 1, 2, -1, -3, hi - zp - 1, lo - zp, hi - zp, 6, -8]
        base = [np_dt((j + 0.5) * s) for j in js]        # exact in float64; the nearest float32 otherwise
        base += [np_dt((lo - zp) * s), np_dt((hi - zp) * s), np_dt((lo - zp - 0.5) * s), np_dt((hi - zp + 0.5) * s),
                 np_dt((lo - zp - 2) * s), np_dt((hi - zp + 2) * s)]
        for b in base:
            vals += [b, np.nextafter(b, np_dt(np.inf)), np.nextafter(b, np_dt(-np.inf))]
    vals = np.array(vals, dtype=np_dt)
    tiny = np.finfo(np_dt).tiny
    special = np.array([0.0, -0.0, np.inf, -np.inf, tiny / 4, -tiny / 4, tiny * 0.75, np.nextafter(np_dt(0), np_dt(1)),
                        1e30, -1e30], dtype=np_dt)
    rng = np.random.default_rng(n_bits * 4 + sym * 2 + one_sided)
    pick = rng.permutation(len(vals))[:N_ROWS - len(special) - 256]
    rest = (rng.standard_normal(N_ROWS - len(special) - len(pick)) * 1.5).astype(np_dt)
    x = np.concatenate([vals[pick], special, rest])
    assert x.shape == (N_ROWS,)
    return torch.from_numpy(x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("one_sided", [False, True], ids=["two_sided", "one_sided"])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
@pytest.mark.parametrize("n_bits", [2, 4, 8, 16])
def test_elements_bit_exact(n_bits, sym, one_sided, dtype):
    import fp8q
    thr = _thresholds()
    x = _adversarial(dtype, thr, sym, n_bits, one_sided)
    ref = _cpu_squares(x, thr, sym, n_bits, one_sided).double().numpy()          # [65, 4096]; the widening is exact
    grid = torch.from_numpy(thr).view(-1, 1).expand(N_K, N_ROWS).contiguous().cuda()
    got = fp8q.ops.int_sse_grid(x.view(N_ROWS, 1).cuda(), True, grid, n_bits, sym, one_sided).cpu().numpy()
    assert got.shape == (N_K, N_ROWS)
    assert not np.isnan(ref).any()                       # no NaN input: nothing to exempt
    bad = np.argwhere(_bits64(got) != _bits64(ref))
    assert bad.size == 0, [(int(k), float(x[r]), float(thr[k]), got[k, r], ref[k, r]) for k, r in bad[:5]]


# ---------------------------------------------------------------------------------------------------------------------
# sums
# ---------------------------------------------------------------------------------------------------------------------
INNERS = [3, 255, 257, 1025, 4097]
NCANDS = [1, 33, 63, 64, 65, 257, 1000]


def _sum_thresholds():
    return np.float32((4.9 + 0.5) * 10.0 / 1000 * np.arange(1, 1001))


@pytest.fixture(scope="module")
def sum_case():
    """dtype -> (buffer [1 + 5 * 4097], exact row sums [inner][1000, 5]) -- computed once, never changed"""
    out = {}
    for dtype in (torch.float32, torch.float64):
        g = torch.Generator().manual_seed(11)
        buf = (torch.randn(1 + 5 * 4097, generator=g, dtype=torch.float64) * 1.3).to(dtype)
        x = buf[1:].view(5, 4097)
        exact = {inner: np.zeros((1000, 5)) for inner in INNERS}
        for k, t in enumerate(_sum_thresholds().tolist()):
            sq = ((x - _candidate(True, 8, False, t)(x)) ** 2).double().numpy()          # [5, 4097]; the widening is exact
            for inner in INNERS:
                exact[inner][k] = [math.fsum(sq[c, :inner].tolist()) for c in range(5)]
        out[dtype] = (buf, exact)
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [1, 5])
@pytest.mark.parametrize("inner", INNERS)
def test_sums_against_fsum(sum_case, inner, C, dtype):
    """Relative error <= (inner + 2) 2^-53 against the exactly summed squares: the terms are non-negative, each addition
    rounds once (inner - 1 of them whatever the order), and one more accumulates into `out`."""
    import fp8q
    buf, exact = sum_case[dtype]
    dev = torch.empty(1 + C * inner, dtype=dtype, device="cuda")
    dev[1:].view(C, inner).copy_(buf[1:].view(5, 4097)[:C, :inner])
    x = dev[1:].view(C, inner)                          # a view one element into its buffer
    assert x.data_ptr() % 16 != 0
    thr = _sum_thresholds()
    for n_cand in NCANDS:
        grid = torch.from_numpy(thr[:n_cand]).view(-1, 1).expand(n_cand, C).contiguous().cuda()
        got = fp8q.ops.int_sse_grid(x, True, grid, 8, True, False).cpu().numpy()
        ref = exact[inner][:n_cand, :C]
        err = np.abs(got - ref) / ref
        print(f"inner={inner} C={C} n_cand={n_cand} max rel err {err.max():.3e} bound {(inner + 2) * U:.3e}")
        assert (ref > 0).all()
        assert (err <= (inner + 2) * U).all(), (n_cand, float(err.max()))


def test_nan_row():
    import fp8q
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 700, generator=g, dtype=torch.float64)
    thr = np.float32(0.05 * np.arange(1, 71))
    grid = torch.from_numpy(thr).view(-1, 1).expand(70, 3).contiguous().cuda()
    clean = fp8q.ops.int_sse_grid(x.cuda(), True, grid).cpu().numpy()
    for dtype in (torch.float64, torch.float32):
        xn = x.to(dtype).clone()
        xn[1, 333] = float("nan")
        want = fp8q.ops.int_sse_grid(x.to(dtype).cuda(), True, grid).cpu().numpy()
        got = fp8q.ops.int_sse_grid(xn.cuda(), True, grid).cpu().numpy()
        assert np.isnan(got[:, 1]).all()
        assert np.array_equal(_bits64(got[:, [0, 2]]), _bits64(want[:, [0, 2]]))
    assert not np.isnan(clean).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_accumulation_and_determinism(sum_case, dtype):
    import fp8q
    buf, exact = sum_case[dtype]
    inner, C, n_cand = 4097, 5, 257
    x = buf.cuda()[1:].view(C, inner)
    grid = torch.from_numpy(_sum_thresholds()[:n_cand]).view(-1, 1).expand(n_cand, C).contiguous().cuda()
    a = fp8q.ops.int_sse_grid(x, True, grid)
    b = fp8q.ops.int_sse_grid(x, True, grid)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))           # two fresh calls: identical bits
    twice = fp8q.ops.int_sse_grid(x, True, grid, out=a.clone())
    ref = 2.0 * exact[inner][:n_cand, :C]
    err = np.abs(twice.cpu().numpy() - ref) / ref
    assert (err <= (inner + 2) * U).all(), float(err.max())


def test_cpu_tensor_is_refused():
    import fp8q
    with pytest.raises(fp8q.Fp8qError):
        fp8q.ops.int_sse_grid(torch.zeros(8), False, torch.ones(3, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own search (tests/golden/g5_quant_error.npz: LineSearchEstimator + SymmetricUniformQuantizer(n_bits=8))
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["uniform", "gauss", "student"])
def test_line_search_losses_equal_the_references(golden_dir, name):
    import fp8q
    from test_oracle_f64 import line_search_sample
    g5 = np.load(os.path.join(golden_dir, "g5_quant_error.npz"))
    x = torch.from_numpy(line_search_sample(name)).cuda()
    assert x.dtype == torch.float64 and x.numel() == 200000
    max_pos_thr, max_search_range, step_size, one_sided = g5[f"{name}_search_0"]
    assert not one_sided
    thr = np.float32(step_size * np.arange(1, 1001))
    loss = g5[f"{name}_loss_0"][0]
    got = fp8q.ops.int_sse_grid(x, False, torch.from_numpy(thr.reshape(-1, 1)).cuda(), 8, True, False).cpu().numpy()[:, 0]
    print(name, "max rel diff", float(np.max(np.abs(got - loss[1:]) / loss[1:])))
    np.testing.assert_allclose(got, loss[1:], rtol=1e-12)
    assert int(np.argmin(got)) + 1 == int(np.argmin(loss))


# ---------------------------------------------------------------------------------------------------------------------
# estimator level
# ---------------------------------------------------------------------------------------------------------------------
EST_CASES = ["f64", "f32", "per_channel", "one_sided", "asym"]


def _est_case(case):
    """(quantizer, per_channel, batches) of an estimator case; CPU tensors"""
    g = torch.Generator().manual_seed(21)
    if case == "f64":
        return _quantizer(True, 8), False, [torch.randn(20000, generator=g, dtype=torch.float64)]
    if case == "f32":
        return _quantizer(True, 8), False, [torch.randn(20000, generator=g)]
    if case == "per_channel":
        scale = torch.tensor([0.5, 1.0, 2.0, 0.7, 1.5, 3.0], dtype=torch.float64).view(6, 1)
        return _quantizer(True, 8, per_channel=True), True, [torch.randn(6, 3000, generator=g, dtype=torch.float64) * scale
                                                              for _ in range(2)]
    if case == "one_sided":
        return _quantizer(True, 8), False, [torch.randn(20000, generator=g, dtype=torch.float64).abs()]
    if case == "asym":
        return _quantizer(False, 8), False, [torch.randn(20000, generator=g, dtype=torch.float64) + 0.25]
    raise KeyError(case)


def _run_est(case):
    from quantization.estimators import LineSearchEstimator
    q, pc, batches = _est_case(case)
    est = LineSearchEstimator(quantizer=q, per_channel=pc)
    for b in batches:
        lo, hi = est(b.cuda())
    return est, lo, hi


def _summary(est, lo, hi):
    return {"argmin": est.loss_array.argmin(axis=1).tolist(), "xmin": lo.cpu().double().reshape(-1).tolist(),
            "xmax": hi.cpu().double().reshape(-1).tolist(), "one_sided": bool(est.one_sided_dist),
            "loss": est.loss_array[:, 1:].tolist()}


@pytest.fixture(scope="module")
def loop_results():
    """every estimator case through the candidate loop: ONE fresh child process with FP8Q_INT_KERNELS=0 (deepcopy calls
    are counted at the top level only: copying a module recurses through copy.deepcopy itself)"""
    code = ("import json, sys, copy\n"
            f"sys.path[:0] = [{os.path.join(ROOT, 'fp8-quantization_amd')!r}, {os.path.join(ROOT, 'tests')!r}, {ROOT!r}]\n"
            "import fp8q.ops as ops, test_int_search_kernels as t\n"
            "calls = {'grid': 0, 'deepcopy': 0}\n"
            "g0, d0 = ops.int_sse_grid, copy.deepcopy\n"
            "def g1(*a, **k):\n    calls['grid'] += 1\n    return g0(*a, **k)\n"
            "def d1(*a, **k):\n    calls['deepcopy'] += len(a) == 1 and not k\n    return d0(*a, **k)\n"
            "ops.int_sse_grid, copy.deepcopy = g1, d1\n"
            "res = {c: t._summary(*t._run_est(c)) for c in t.EST_CASES}\n"
            "res['calls'] = calls\n"
            "print('RESULT' + json.dumps(res))\n")
    env = dict(os.environ, FP8Q_INT_KERNELS="0")
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):])


def test_child_process_takes_the_loop(loop_results):
    n_batches = sum(len(_est_case(c)[2]) for c in EST_CASES)
    assert loop_results["calls"]["grid"] == 0
    assert loop_results["calls"]["deepcopy"] == 1000 * n_batches


@pytest.mark.parametrize("case", EST_CASES)
def test_estimator_one_call_per_batch(loop_results, monkeypatch, case):
    import copy
    import fp8q
    calls = {"grid": 0, "deepcopy": 0}
    real_grid, real_deepcopy = fp8q.ops.int_sse_grid, copy.deepcopy

    def counted_grid(*a, **k):
        calls["grid"] += 1
        return real_grid(*a, **k)

    def counted_deepcopy(*a, **k):
        calls["deepcopy"] += len(a) == 1 and not k
        return real_deepcopy(*a, **k)

    monkeypatch.setattr(fp8q.ops, "int_sse_grid", counted_grid)
    monkeypatch.setattr(copy, "deepcopy", counted_deepcopy)
    monkeypatch.delenv("FP8Q_INT_KERNELS", raising=False)
    est, lo, hi = _run_est(case)
    n_batches = len(_est_case(case)[2])
    assert calls == {"grid": n_batches, "deepcopy": 0}
    got, want = _summary(est, lo, hi), loop_results[case]
    assert got["argmin"] == want["argmin"]
    assert got["xmin"] == want["xmin"] and got["xmax"] == want["xmax"]
    assert got["one_sided"] == want["one_sided"] == (case == "one_sided")
    if case == "one_sided":
        assert got["xmin"] == [0.0]
    if case == "per_channel":
        assert len(got["argmin"]) == 6 and len(set(got["argmin"])) > 1
    if case != "f32":      # (the loop sums float32 squares in float32; float64 ones in ATen's order: close, not equal)
        np.testing.assert_allclose(got["loss"], want["loss"], rtol=1e-9)
