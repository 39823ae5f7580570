"""The contract of the half-precision lane, pinned on the CPU: the reference's own outputs for float16 / bfloat16
inputs (tests/golden/gh1_half.npz, made by tests/golden/make_golden_h16.py) are what the EXISTING fp32 oracle gives on
the exactly widened input -- same metric as tests/test_oracle_golden.py uses for the fp32 fixtures (at most 2 fp32 ULP,
no grid-step flips).  Needs no kernel: it shows that `oracle(x.float())` is the right yardstick for the GPU tests."""
import os

import numpy as np
import pytest
import torch

import oracle
from parity import assert_parity, elem_step

DT = {0: torch.float16, 1: torch.bfloat16}


@pytest.fixture(scope="module")
def gh1(golden_dir):
    return np.load(os.path.join(golden_dir, "gh1_half.npz"))


def _widen(bits, dtype):
    return torch.from_numpy(bits.view(np.int16).copy()).view(dtype).float().numpy()


def test_fixture_is_small_and_complete(golden_dir, gh1):
    assert os.path.getsize(os.path.join(golden_dir, "gh1_half.npz")) < 500 * 1024
    cases = gh1["cases"]
    seen = {(int(d), int(pc), int(nb), int(M), int(s)) for _, d, pc, nb, M, s in cases}
    for d in (0, 1):
        for pc in (0, 1):
            for fmt in ((8, 2, 1), (8, 3, 1), (8, 4, 1), (8, 3, 0), (6, 2, 1)):
                assert (d, pc) + fmt in seen


def test_oracle_on_widened_input_vs_reference(gh1):
    tot, exact = 0, 0.0
    for cid, d, pc, n_bits, M, s in gh1["cases"]:
        x = _widen(gh1[f"c{cid}_x"], DT[int(d)])
        mv, y_ref = gh1[f"c{cid}_maxval"], gh1[f"c{cid}_y"]
        assert y_ref.dtype == np.float32 and x.shape == y_ref.shape
        assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any()          # the edge inputs are there
        y = oracle.c_quantize(x, mv, float(M), int(n_bits), int(s))
        assert np.array_equal(np.isnan(y), np.isnan(y_ref)), f"case {cid}: NaN placement"
        ok = ~np.isnan(y_ref)
        step = elem_step(x, mv, float(M), int(n_bits), int(s))
        yr, rr, sr = (np.where(ok, a, 0.0).astype(np.float32) for a in (y, y_ref, step))
        r = assert_parity(yr, rr, np.where(ok, sr, 1.0).astype(np.float32), max_flip_frac=0.0, max_ulp=2, what=f"case {cid}")
        tot += r["n"]
        exact += r["exact_frac"] * r["n"]
    print(f"\noracle(widen(x)) vs reference on half inputs: {tot} elements, bit-exact {exact / tot:.4%}")
    assert exact / tot > 0.90


def test_minmax_ranges_vs_reference(gh1):
    """Ranges bit-equal, for all three estimators and every batch, against both records of the fixture:
      - the reference on the widened batches (x.float(); estimates and fold in float32) equals the oracle's min/max and
        fp32 fold bit for bit -- this is the lane's contract: the running estimate of a half tensor is kept in float32;
      - the reference on the half batches as they are keeps its estimates in the input's dtype.  min and max are exact
        in any precision, so current_minmax / allminmax equal the oracle's fp32 values bit for bit; running_minmax folds
        (1 - m) * new + m * cur in the half type, and that very sequence -- three separately rounded half operations on
        the oracle's (exactly representable) min / max -- reproduces the fixture bit for bit, which shows that the two
        records differ by nothing but the precision of the fold."""
    for dname, dtype in (("f16", torch.float16), ("bf16", torch.bfloat16)):
        for pc in (0, 1):
            xs = [_widen(b, dtype) for b in gh1[f"mm_{dname}_pc{pc}_x"]]
            for ename, mode in (("current_minmax", 0), ("allminmax", 1), ("running_minmax", 2)):
                key = f"mm_{dname}_pc{pc}_{ename}"
                ref_min, ref_max, w_min, w_max = gh1[key + "_min"], gh1[key + "_max"], gh1[key + "_wmin"], gh1[key + "_wmax"]
                assert str(gh1[key + "_dtype"][0]) == str(dtype)
                cur = half_cur = None
                for b, x in enumerate(xs):
                    mn, mx = oracle.c_minmax(x, bool(pc))
                    hmn, hmx = torch.from_numpy(mn).to(dtype), torch.from_numpy(mx).to(dtype)
                    assert np.array_equal(hmn.float().numpy().view(np.int32), mn.view(np.int32))      # exact in the half type
                    if cur is not None:
                        fmn, fmx = oracle.c_fold(cur[0], cur[1], mn, mx, mode, 0.9)
                        if mode == 2:     # range_estimators.py:122-123 on half tensors
                            hmn = (1 - 0.9) * hmn + 0.9 * half_cur[0]
                            hmx = (1 - 0.9) * hmx + 0.9 * half_cur[1]
                        else:
                            hmn, hmx = torch.from_numpy(fmn).to(dtype), torch.from_numpy(fmx).to(dtype)
                        mn, mx = fmn, fmx
                    cur, half_cur = (mn, mx), (hmn, hmx)
                    what = (dname, pc, ename, b)
                    assert np.array_equal(mn.view(np.int32), w_min[b].view(np.int32)), what
                    assert np.array_equal(mx.view(np.int32), w_max[b].view(np.int32)), what
                    assert np.array_equal(hmn.float().numpy().view(np.int32), ref_min[b].view(np.int32)), what
                    assert np.array_equal(hmx.float().numpy().view(np.int32), ref_max[b].view(np.int32)), what
                    if mode != 2:
                        assert np.array_equal(mn.view(np.int32), ref_min[b].view(np.int32)), what
                        assert np.array_equal(mx.view(np.int32), ref_max[b].view(np.int32)), what
