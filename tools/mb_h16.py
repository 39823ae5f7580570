#!/usr/bin/env python
"""Micro-benchmark of the half-precision lane (csrc/fp8q_h16.hip) on the headline tensor [2^21, 3, 7, 7], E5M2, fixed
ranges, per channel and per tensor, for float16 and bfloat16, all in one process:

  fp32 K1                         fp8q_quantize_f32                               8 B / element
  half in -> fp32 out             fp8q_quantize_h16, y_type = FP8Q_DT_F32         6
  half in -> half out             fp8q_quantize_h16, y_type = x_type              4
  min/max + quantize (half out)   fp8q_minmax_quantize_h16 (per channel)          6   (2 B scan + 4 B K1)
  min/max scan                    fp8q_minmax_h16                                 2
  widen, fp32 K1, narrow          ops.quantize(x.float(), ...).to(x.dtype)        20  (2+4, 4+4, 4+2): the only route
                                  half data had before this lane existed

Time per call by HIP events (median of 20 after a warm-up), GB/s over the algorithmic bytes and the fraction of 8 TB/s.
The last column of the half in -> half out line is its speed-up over the widen-quantize-narrow chain timed in the same
run; 2.5 x (half the byte ratio 20 / 4) is the requirement.

    python tools/mb_h16.py [--quick] > profiles/h16_mb.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

HBM = 8.0e12
SHAPE = (1 << 21, 3, 7, 7)


def _events(fn, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def _line(name, t, nbytes, extra=""):
    print(f"  {name:34s} {t * 1e6:9.1f} us  {nbytes / t / 1e9:8.1f} GB/s  {nbytes / t / HBM:5.3f} of 8 TB/s{extra}")
    return t


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    print(torch.cuda.get_device_name(0))
    print(f"tensor {list(SHAPE)}, E5M2 (n_bits 8, M 2, sign 1), fixed ranges; median of {reps} by HIP events")
    n = 1
    for s in SHAPE:
        n *= s
    x32 = torch.randn(SHAPE, device="cuda")
    worst = None
    for pc in (True, False):
        mv = (x32.view(SHAPE[0], -1).abs().amax(1) * 0.9).contiguous() if pc else torch.tensor([2.5], device="cuda")
        print(f"{'per channel' if pc else 'per tensor'}:")
        y32 = torch.empty_like(x32)
        t32 = _line("fp32 K1", _events(lambda: ops.quantize(x32, mv, 2.0, 8, 1, out=y32), reps), 8.0 * n)
        del y32
        for dt in (torch.bfloat16, torch.float16):
            x = x32.to(dt)
            name = str(dt).replace("torch.", "")
            yf = torch.empty(SHAPE, dtype=torch.float32, device="cuda")
            _line(f"{name} in -> fp32 out", _events(lambda: ops.quantize(x, mv, 2.0, 8, 1, out=yf), reps), 6.0 * n)
            del yf
            yh = torch.empty_like(x)
            th = _events(lambda: ops.quantize(x, mv, 2.0, 8, 1, out=yh), reps)
            tc = _events(lambda: ops.quantize(x.float(), mv, 2.0, 8, 1).to(dt), reps)
            _line(f"{name} in -> {name} out", th, 4.0 * n, f"   {tc / th:4.2f}x the chain below (fp32 K1 {t32 / th:4.2f}x)")
            _line(f"{name} widen, fp32 K1, narrow", tc, 20.0 * n)
            if pc:
                _line(f"{name} min/max + quantize", _events(lambda: ops.minmax_quantize(x, 2.0, 8, 1, out=yh), reps), 6.0 * n)
            _line(f"{name} min/max scan", _events(lambda: ops.minmax(x, pc), reps), 2.0 * n)
            worst = tc / th if worst is None else min(worst, tc / th)
            del x, yh
            torch.cuda.empty_cache()
    ops.check_workspaces()
    print(f"smallest speed-up of half in -> half out over the widen-quantize-narrow chain: {worst:4.2f}x "
          f"(required: 2.5x) -> {'met' if worst >= 2.5 else 'NOT met'}")
    return 0 if worst >= 2.5 else 1


if __name__ == "__main__":
    sys.exit(main())
