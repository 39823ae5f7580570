#!/usr/bin/env python
"""Micro-benchmark of the uniform (INT) quantizers on half tensors (csrc/fp8q_inth16.hip): INT8, fixed ranges, symmetric and
asymmetric, for bfloat16 and float16, on the weight-shaped tensor [2^21, 3, 7, 7] per channel and the activation-shaped
tensor [64, 64, 112, 112] per tensor, all in one process:

  half in -> half out             fp8q_int_quantize_h16, y_type = x_type              4 B / element
  half in -> fp32 out             fp8q_int_quantize_h16, y_type = FP8Q_DT_F32         6
  widen, fp32 kernel, narrow      ops.int_quantize(x.float(), ...).to(x.dtype)        20  (2+4, 4+4, 4+2): the only route
                                  half data had before this lane existed
  fp32 kernel                     fp8q_int_quantize_f32 on float32 data               8

Time per call by HIP events (median of 20 after a warm-up), GB/s over the algorithmic bytes and the fraction of 8 TB/s.
The last column of the half in -> half out line is its speed-up over the widen-quantize-narrow chain timed in the same run.
There is no target: the file reports what was measured, faster or slower.

    python tools/mb_int_h16.py [--quick] [--out profiles/int_h16_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

HBM = 8.0e12
CASES = [((1 << 21, 3, 7, 7), True), ((64, 64, 112, 112), False)]


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


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int_h16_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def line(name, t, nbytes, extra=""):
        emit(f"  {name:34s} {t * 1e6:9.1f} us  {nbytes / t / 1e9:8.1f} GB/s  {nbytes / t / HBM:5.3f} of 8 TB/s{extra}")

    emit(torch.cuda.get_device_name(0))
    emit(f"INT8 (n_bits 8), fixed ranges; median of {reps} by HIP events")
    ratios = []
    for shape, pc in CASES:
        n = 1
        for s in shape:
            n *= s
        x32 = torch.randn(shape, device="cuda")
        C = shape[0] if pc else 1
        lo = x32.view(C, -1).amin(1).contiguous()
        hi = x32.view(C, -1).amax(1).contiguous()
        for symmetric in (True, False):
            d, z, sg = ops.int_set_range(lo, hi, 8, symmetric)
            emit(f"{list(shape)}, {'per channel' if pc else 'per tensor'}, {'symmetric' if symmetric else 'asymmetric'}:")
            y32 = torch.empty_like(x32)
            t32 = _events(lambda: ops.int_quantize(x32, d, z, sg, 8, symmetric, out=y32), reps)
            line("fp32 kernel", t32, 8.0 * n)
            del y32
            for dt in (torch.bfloat16, torch.float16):
                x = x32.to(dt)
                name = str(dt).replace("torch.", "")
                yh = torch.empty_like(x)
                th = _events(lambda: ops.int_quantize(x, d, z, sg, 8, symmetric, out=yh), reps)
                tc = _events(lambda: ops.int_quantize(x.float(), d, z, sg, 8, symmetric).to(dt), reps)
                line(f"{name} in -> {name} out", th, 4.0 * n, f"   {tc / th:4.2f}x the chain below (fp32 kernel {t32 / th:4.2f}x)")
                line(f"{name} widen, fp32 kernel, narrow", tc, 20.0 * n)
                del yh
                yf = torch.empty(shape, dtype=torch.float32, device="cuda")
                line(f"{name} in -> fp32 out", _events(lambda: ops.int_quantize(x, d, z, sg, 8, symmetric, out=yf), reps), 6.0 * n)
                ratios.append(tc / th)
                del x, yf
                torch.cuda.empty_cache()
        del x32
        torch.cuda.empty_cache()
    emit(f"half in -> half out over the widen-quantize-narrow chain: {min(ratios):4.2f}x to {max(ratios):4.2f}x "
         f"({'faster in every case' if min(ratios) > 1 else 'NOT faster in every case'})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
