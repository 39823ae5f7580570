#!/usr/bin/env python
"""Print the table "op / kernel / variant -> shapes that reach it" of the row kernels' test shapes (tests/rows_cases.py) as
ops.rows_route reports them: host arithmetic only, needs the built library and no GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fp8-quantization_amd"), ROOT):
    sys.path.insert(0, p)

import rows_cases as rc          # noqa: E402
from fp8q import ops             # noqa: E402


def main():
    reached = {}
    for key in rc.build_shapes(ops):
        r = rc.route_of(ops, key)
        reached.setdefault((key[0], r["kernel"], rc.variant(key, r)), []).append(key)
    print("# Row kernels: the test shapes that reach each kernel and variant\n")
    print("Written by `tools/rows_route_table.py` (shapes: `tests/rows_cases.py`; routes: `ops.rows_route`).  A shape is")
    print("`[C,inner]`, then the format `(mbits,n_bits,sign_bits)` unless E5M2, `x+k`/`y+k` for pointers k elements off a")
    print("16-byte boundary, `ip` for in place.\n")
    print("| op | kernel | variant | shapes |\n|---|---|---|---|")
    for v in sorted(reached):
        cells = []
        for op, C, inner, fmt, xp, yp, ip in reached[v]:
            c = "[%d,%d]" % (C, inner) + ("" if fmt == rc.E5M2 else " (%g,%d,%d)" % fmt)
            c += (" x+%d" % xp if xp else "") + (" y+%d" % yp if yp and not ip and rc.base_op(op) != "minmax" else "") + (" ip" if ip else "")
            cells.append(c)
        print("| %s | %s | %s | %s |" % (v[0], v[1], v[2] or "-", "; ".join(cells)))


if __name__ == "__main__":
    main()
