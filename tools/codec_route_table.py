#!/usr/bin/env python
"""Print the table "direction / kernel / variant -> shapes that reach it" of the storage-code kernels' test shapes
(tests/codec_cases.py) as ops.codec_route reports them: host arithmetic only, needs the built library and no GPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fp8-quantization_amd"), ROOT):
    sys.path.insert(0, p)

import codec_cases as cc         # noqa: E402
from fp8q import ops             # noqa: E402


def main():
    reached = {}
    for key in cc.build_shapes(ops):
        r = cc.route_of(ops, key)
        for v in cc.variant(key, r):
            reached.setdefault(("encode" if key[0] else "decode", r["kernel"], v), []).append(key)
    print("# Storage codes: the test shapes that reach each kernel and variant\n")
    print("Written by `tools/codec_route_table.py` (shapes: `tests/codec_cases.py`; routes: `ops.codec_route`).  A shape is")
    print("`[C,inner]`, then the format `(mbits,n_bits,sign_bits)` unless E5M2, `f+k` for a float32 side k elements and `c+k` for")
    print("codes k bytes off a 16-byte boundary, `pt` for one range per tensor.\n")
    print("| direction | kernel | variant | shapes |\n|---|---|---|---|")
    for v in sorted(reached):
        cells = []
        for enc, C, inner, fmt, fp, cp, pc in reached[v]:
            c = "[%d,%d]" % (C, inner) + ("" if fmt == cc.E5M2 else " (%g,%d,%d)" % fmt)
            c += (" f+%d" % fp if fp else "") + (" c+%d" % cp if cp else "") + ("" if pc else " pt")
            cells.append(c)
        print("| %s | %s | %s | %s |" % (v[0], v[1], v[2], "; ".join(cells)))


if __name__ == "__main__":
    main()
