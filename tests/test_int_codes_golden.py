"""to_integer_forward of the uniform (INT) quantizers against the REFERENCE (tests/golden/gu2_uniform_int.npz, written by
tests/golden/make_golden_int_codes.py from the reference's to_integer_forward on gu1_uniform.npz's inputs and
current_minmax ranges).  CPU: this repository's eager chain on gu1's recorded delta / zero_float / signed buffers, bit for
bit with NaN at the same places -- which pins the chain that the kernel tests (tests/test_int_codes_kernels.py) compare
against."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(q, pc, nb) for q in ("sym", "asym") for pc in (0, 1) for nb in (2, 4, 8, 16)]


@pytest.fixture(scope="module")
def gu():
    return np.load(os.path.join(HERE, "golden", "gu1_uniform.npz")), np.load(os.path.join(HERE, "golden", "gu2_uniform_int.npz"))


def _eq_nan(got, want):
    got = np.ascontiguousarray(np.asarray(got, dtype=np.float32))
    want = np.ascontiguousarray(np.asarray(want, dtype=np.float32))
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32))


def test_the_fixture_covers_every_case_of_gu1(gu):
    g1, g2 = gu
    assert sorted(g2.files) == sorted(f"{q}_pc{pc}_b{nb}_t" for q, pc, nb in CASES)
    for q, pc, nb in CASES:
        t = g2[f"{q}_pc{pc}_b{nb}_t"]
        assert t.dtype == np.float32 and t.shape == g1[f"{q}_pc{pc}_b{nb}_x"].shape
        v = t[~np.isnan(t)]
        assert np.array_equal(v, np.rint(v)) and v.min() >= -(2.0 ** (nb - 1)) and v.max() <= 2.0 ** nb - 1


@pytest.mark.parametrize("qname,pc,nb", CASES)
def test_eager_to_integer_forward_on_cpu_equals_the_reference(gu, qname, pc, nb):
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    g1, g2 = gu
    case = f"{qname}_pc{pc}_b{nb}"
    rec = case + "_current_minmax"
    for i, x in enumerate(g1[case + "_x"]):
        q = (SymmetricUniformQuantizer if qname == "sym" else AsymmetricUniformQuantizer)(n_bits=nb, per_channel=bool(pc))
        q._delta = torch.from_numpy(g1[rec + "_delta"][i].copy())
        if qname == "sym":
            q._signed = torch.tensor(bool(g1[rec + "_signed"][i]))
        else:
            q._zero_float = torch.from_numpy(g1[rec + "_zf"][i].copy())
        t = q.to_integer_forward(torch.from_numpy(x))
        assert _eq_nan(t.numpy(), g2[case + "_t"][i]), (case, i)
