// Stand-alone host check of the percentile contract's rank computation (csrc/fp8q_percentile_ranks.h), meant for a
// sanitizer build on the CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cabi/percentile_ranks_main.cpp -o ranks && ./ranks
// Exits non-zero when an invariant of include/fp8q.h ("Percentile ranges", step 2) fails.
#include <stdio.h>

#include "../../fp8-quantization_amd/csrc/fp8q_percentile_ranks.h"

static int check(double q, int64_t n, const char *what)
{
    int64_t k = -1, k1 = -1;
    double t = -1.0;
    fp8q_percentile_rank(q, n, &k, &k1, &t);
    const double pos = q * (double)(n - 1);
    int bad = 0;
    bad |= !(k >= 0 && k <= n - 1);
    bad |= !(k1 == (k + 1 < n ? k + 1 : n - 1));
    bad |= !(t >= 0.0 && t < 1.0);
    bad |= !((double)k + t == pos);
    if (q == 0.0) bad |= !(k == 0 && t == 0.0);
    if (q == 1.0) bad |= !(k == n - 1 && k1 == n - 1 && t == 0.0);
    if (bad) fprintf(stderr, "FAIL %s q=%.17g n=%lld: k=%lld k1=%lld t=%.17g\n", what, q, (long long)n, (long long)k, (long long)k1, t);
    return bad;
}

int main()
{
    const int64_t ns[] = {1, 2, 3, ((int64_t)1 << 24) + 1, (int64_t)1 << 40};
    const double pcts[] = {0.01, 0.1, 1.0, 5.0, 50.0, 0.0, 100.0, 50.5, 63.0, 99.9};
    int bad = 0, cases = 0;
    for (int64_t n : ns)
        for (double pct : pcts) {
            bad += check(pct / 100.0, n, "lo");
            bad += check((100.0 - pct) / 100.0, n, "hi");
            cases += 2;
        }
    printf("%d cases, %d failures\n", cases, bad);
    return bad ? 1 : 0;
}
