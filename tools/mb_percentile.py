#!/usr/bin/env python
"""Micro-benchmark of the percentile selection (csrc/fp8q_select.hip, fp8q.ops.percentile) on the shapes the estimator meets:

  per channel   [2^21, 3, 7, 7]  and  [58254, 512, 3, 3]      row-resident route, x read once: 4 B / element
  per tensor    [64, 64, 56, 56] and  [64, 64, 112, 112]      streaming route, x read three times: 12 B / element

Time per call by HIP events (median of `reps` after a warm-up), bytes moved / time as a fraction of 8 TB/s, and -- where
torch.quantile accepts the tensor (it refuses more than 2^24 elements) -- the estimator's torch.quantile branch (float64 copy +
library sort) timed in the same process, with the ratio.

    python tools/mb_percentile.py [--quick] [--out profiles/percentile_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

from mb_grad import _events  # noqa: E402

HBM = 8e12
CASES = [((1 << 21, 3, 7, 7), True), ((58254, 512, 3, 3), True), ((64, 64, 56, 56), False), ((64, 64, 112, 112), False)]
PCT = 0.1


def _quantile_branch(x, per_channel):
    f = x.reshape(x.shape[0], -1) if per_channel else x.reshape(-1)
    q = torch.tensor([PCT / 100.0, 1 - PCT / 100.0], device=x.device, dtype=torch.float64)
    return torch.quantile(f.double(), q, dim=-1).float()


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "percentile_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    R = ops.percentile_resident_max_inner()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"percentile {PCT}: lo / hi per row; median of {reps} by HIP events; rows up to {R} elements are row-resident")
    for shape, pc in CASES:
        n = 1
        for s in shape:
            n *= s
        inner = n // shape[0] if pc else n
        x = torch.randn(shape, device="cuda")
        route, per_el = ("row-resident", 4) if inner <= R else ("streaming", 12)
        say(f"{list(shape)} {'per channel' if pc else 'per tensor'} ({n} elements, {route}, {per_el} B / element):")
        t = _events(lambda: ops.percentile(x, pc, PCT), reps)
        say(f"  ops.percentile        {t * 1e6:10.1f} us  {per_el * n / t / 1e12:6.3f} TB/s  {per_el * n / t / HBM:5.3f} of 8 TB/s")
        try:
            tq = _events(lambda: _quantile_branch(x, pc), max(3, reps // 4))
            say(f"  torch.quantile branch {tq * 1e6:10.1f} us  {tq / t:7.1f} x ops.percentile's time")
        except RuntimeError as e:
            say(f"  torch.quantile branch: no baseline, it raises ({str(e).splitlines()[0][:70]})")
        del x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
