// fp8q_percentile_ranks.h -- host side of the percentile contract (include/fp8q.h, "Percentile ranges"): the ranks and the
// interpolation weight of one quantile of a row of n elements.  Plain C++, no HIP: fp8q_select.hip includes it, and so does
// the stand-alone sanitizer program tests/cabi/percentile_ranks_main.cpp.
#pragma once
#include <math.h>
#include <stdint.h>

// pos = q (n - 1) in double; k = clamp(floor(pos), 0, n - 1), k1 = min(k + 1, n - 1), t = pos - k.  n >= 1, 0 <= q <= 1.
inline void fp8q_percentile_rank(double q, int64_t n, int64_t *k, int64_t *k1, double *t)
{
    const double pos = q * (double)(n - 1);
    double fl = floor(pos);
    if (!(fl >= 0.0)) fl = 0.0;                               // (also a NaN pos: the entry point refuses it before)
    if (fl > (double)(n - 1)) fl = (double)(n - 1);           // clamped in double: the cast below never overflows
    int64_t kk = (int64_t)fl;
    if (kk > n - 1) kk = n - 1;                               // (double)(n - 1) may round up for n > 2^53
    *k = kk;
    *k1 = kk + 1 < n ? kk + 1 : n - 1;
    *t = pos - (double)kk;
}
