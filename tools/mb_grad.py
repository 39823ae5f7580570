#!/usr/bin/env python
"""Micro-benchmark of the FP quantizer's backward (csrc/fp8q_grad.hip) against the torch chain it replaces
(FP8Q_GRAD_KERNELS=0: the parent's backward) on the same buffers, E5M2, per tensor and per channel, on the headline tensor
[2^21, 3, 7, 7] and on conv1's [64, 3, 7, 7], all in one process:

  kernel, gx + gmaxval             fp8q_quantize_bwd_f32                           12 B / element (x, g in; gx out)
  kernel, gmaxval only                                                              8
  forward + backward, both routes  quantize_to_fp8_ste_MM(x, maxval).backward(g) with x and maxval requiring a gradient:
                                   the kernel route, and the torch chain (_FakeQuantSTE.backward on the saved y, ~25 ATen
                                   launches, > 60 B / element); their peak memory (the kernel route does not keep y)

Time per call by HIP events (median of 20 after a warm-up), GB/s over the algorithmic bytes and the fraction of 8 TB/s.
Requirement: the kernel route is faster than the chain on every shape.  The verdict compares like with like: forward +
backward through autograd on either route, the same host work on both sides.  The bare kernel call is listed on its own; the
chain's backward alone (its forward + backward minus the bare forward kernel, so it still carries autograd's host overhead,
which dominates on the small tensor) is given for orientation and does not enter the verdict.

    python tools/mb_grad.py [--quick] > profiles/grad_mb.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

HBM = 8.0e12
SHAPES = [(1 << 21, 3, 7, 7), (64, 3, 7, 7)]


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


def _line(name, t, nbytes=None, extra=""):
    bw = f"{nbytes / t / 1e9:8.1f} GB/s  {nbytes / t / HBM:5.3f} of 8 TB/s" if nbytes else " " * 31
    print(f"  {name:34s} {t * 1e6:9.1f} us  {bw}{extra}")
    return t


def _chain_backward(x, g, mv):
    """one forward + backward through autograd (the route is chosen by FP8Q_GRAD_KERNELS at the forward)"""
    from quantization.fp8 import quantize_to_fp8_ste_MM

    def step():
        xt, mt = x.detach().requires_grad_(True), mv.detach().requires_grad_(True)
        quantize_to_fp8_ste_MM(xt, 8, mt, 2.0, 1).backward(g)
    return step


def _peak(step):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    print(torch.cuda.get_device_name(0))
    print(f"E5M2 (n_bits 8, M 2, sign 1), fixed ranges; median of {reps} by HIP events")
    worst = None
    for shape in SHAPES:
        n = 1
        for s in shape:
            n *= s
        x = torch.randn(shape, device="cuda")
        g = torch.randn(shape, device="cuda")
        for pc in (True, False):
            mv = (x.view(shape[0], -1).abs().amax(1) * 0.9).contiguous() if pc else torch.tensor([2.5], device="cuda")
            print(f"{list(shape)} {'per channel' if pc else 'per tensor'}:")
            y = torch.empty_like(x)
            tf = _line("forward K1 (for orientation)", _events(lambda: ops.quantize(x, mv, 2.0, 8, 1, out=y), reps), 8.0 * n)
            del y
            tk = _events(lambda: ops.quantize_backward(x, g, mv, 2.0, 8, 1, True, True, False), reps)
            t8 = _events(lambda: ops.quantize_backward(x, g, mv, 2.0, 8, 1, False, True, False), reps)
            step = _chain_backward(x, g, mv)
            saved = os.environ.get("FP8Q_GRAD_KERNELS")
            try:
                os.environ["FP8Q_GRAD_KERNELS"] = "0"
                tc_fb = _events(step, reps)
                peak_c = _peak(step)
                os.environ["FP8Q_GRAD_KERNELS"] = "1"
                tk_fb = _events(step, reps)
                peak_k = _peak(step)
            finally:
                if saved is None:
                    os.environ.pop("FP8Q_GRAD_KERNELS", None)
                else:
                    os.environ["FP8Q_GRAD_KERNELS"] = saved
            tc = tc_fb - tf                  # orientation only: the chain's backward with autograd's host overhead
            _line("kernel, gx + gmaxval", tk, 12.0 * n)
            _line("kernel, gmaxval only", t8, 8.0 * n)
            _line("forward + backward, kernel route", tk_fb, None, f"   peak memory {peak_k / 1e6:9.2f} MB   "
                                                                    f"{tc_fb / tk_fb:5.2f}x faster than the torch chain")
            _line("forward + backward, torch chain", tc_fb, None, f"   peak memory {peak_c / 1e6:9.2f} MB  "
                                                                   f"(+{(peak_c - peak_k) / n:4.1f} B / element)")
            _line("(chain minus the bare forward)", tc, None, f"   (the time {tc * HBM / n:4.0f} B / element take at 8 TB/s)")
            worst = tc_fb / tk_fb if worst is None else min(worst, tc_fb / tk_fb)
        del x, g
        torch.cuda.empty_cache()
    print(f"smallest speed-up of forward + backward on the kernel route over the torch chain: {worst:4.2f}x (required: faster on every shape) -> "
          f"{'met' if worst > 1.0 else 'NOT met'}")
    return 0 if worst > 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
