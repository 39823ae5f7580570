"""Host oracle of the percentile contract (include/fp8q.h, "Percentile ranges"): numpy only.  The rows' monotone uint32 keys are
sorted once (np.sort on the transformed bits); ranges(pct) applies steps 2-4 of the contract in float64."""
import math

import numpy as np


def keys_of(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))


def values_of(k):
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def ranks(q, n):
    """(k, k1, t) of quantile q in [0, 1] for a row of n elements; python floats are doubles"""
    pos = q * float(n - 1)
    k = min(max(int(math.floor(pos)), 0), n - 1)
    return k, min(k + 1, n - 1), pos - float(k)


def exact_pct(n, frac=0.37):
    """a percentile whose lower position pct / 100 * (n - 1) is an exact integer in double (t == 0), or None"""
    if n < 3:
        return 0.0
    for j in range(max(1, int(frac * (n - 1))), n - 1):
        pct = 100.0 * j / (n - 1)
        if (pct / 100.0) * float(n - 1) == float(j):
            return pct
    return None


class Oracle:
    def __init__(self, x2d):
        x2d = np.ascontiguousarray(x2d, dtype=np.float32)
        assert x2d.ndim == 2
        self.n = x2d.shape[1]
        self.nan = np.isnan(x2d).any(axis=1)
        self.sorted_keys = np.sort(keys_of(x2d), axis=1)

    def pair(self, q):
        """(a, b, t): the two order statistics of quantile q (float32 [C]) and the weight"""
        k, k1, t = ranks(q, self.n)
        return values_of(self.sorted_keys[:, k]), values_of(self.sorted_keys[:, k1]), t

    def quantile(self, q):
        a, b, t = self.pair(q)
        with np.errstate(all="ignore"):
            d = (b - a).astype(np.float32).astype(np.float64)        # float32 subtraction, one rounding
            v = a.astype(np.float64) + d * t if t < 0.5 else b.astype(np.float64) - d * (1.0 - t)
            out = v.astype(np.float32)
        out[self.nan] = np.nan
        return out

    def ranges(self, pct):
        return self.quantile(pct / 100.0), self.quantile((100.0 - pct) / 100.0)


def assert_bits(got, want, what=""):
    """bit for bit, as integers; a NaN matches any NaN (the contract says NaN, not which one)"""
    got = np.asarray(got, dtype=np.float32).reshape(-1)
    want = np.asarray(want, dtype=np.float32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN rows differ", np.flatnonzero(gn != wn)[:8])
    g, w = got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, (what, bad[:8], got[~gn][bad[:8]], want[~wn][bad[:8]])
