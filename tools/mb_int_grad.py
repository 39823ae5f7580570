#!/usr/bin/env python
"""Micro-benchmark of the INT quantizers' backward (csrc/fp8q_intgrad.hip) against the torch chain it replaces
(FP8Q_GRAD_KERNELS=0: the parent's behaviour) on the same buffers, next to the FP quantizer's backward kernel on the same
tensors: the activation [64, 64, 112, 112] per tensor (asymmetric, 8 bit) and the weight [512, 512, 3, 3] per channel
(symmetric, 8 bit), all in one process:

  kernel, gx + range gradients     fp8q_int_quantize_bwd_f32                       12 B / element (x, g in; gx out)
  kernel, range gradients only                                                      8
  FP kernel, gx + gmaxval          fp8q_quantize_bwd_f32 (E5M2) on the same x and g 12
  forward + backward, both routes  quantizer(x).backward(g) with x and the learned ranges requiring a gradient: the kernel
                                   route, and the torch chain (~8 ATen launches forward, autograd's backward of them)

Time per call by HIP events (median of 20 after a warm-up), TB/s over the algorithmic bytes.

    python tools/mb_int_grad.py [--quick] > profiles/int_grad_mb.txt
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

from mb_grad import _events, _peak  # noqa: E402

CASES = [((64, 64, 112, 112), False), ((512, 512, 3, 3), True)]


def _line(name, t, nbytes=None, extra=""):
    bw = f"{nbytes / t / 1e12:6.3f} TB/s" if nbytes else " " * 11
    print(f"  {name:36s} {t * 1e6:9.1f} us  {bw}{extra}")
    return t


def main():
    from fp8q import ops
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    print(torch.cuda.get_device_name(0))
    print(f"INT8, learned ranges at 0.7 x min / max; median of {reps} by HIP events; TB/s over 12 (8) B / element")
    worst = None
    for shape, pc in CASES:
        n = 1
        for s in shape:
            n *= s
        x = torch.randn(shape, device="cuda")
        g = torch.randn(shape, device="cuda")
        q = (SymmetricUniformQuantizer if pc else AsymmetricUniformQuantizer)(n_bits=8, per_channel=pc)
        rows = x.view(shape[0], -1) if pc else x.view(1, -1)
        q.set_quant_range((rows.amin(1) * 0.7).contiguous(), (rows.amax(1) * 0.7).contiguous())
        q.make_range_trainable()
        d, z, sg = q._delta, (None if pc else q._zero_float), (q._signed if pc else None)
        mv = (rows.abs().amax(1) * 0.7).contiguous()
        print(f"{list(shape)} {'per channel, symmetric' if pc else 'per tensor, asymmetric'}:")
        bwd = lambda gx: ops.int_quantize_backward(x, g, d, z, sg, 8, pc, 1e-8, gx, True, not pc)
        tk = _events(lambda: bwd(True), reps)
        t8 = _events(lambda: bwd(False), reps)
        tfp = _events(lambda: ops.quantize_backward(x, g, mv, 2.0, 8, 1, True, True, False), reps)

        def step():
            xt = x.detach().requires_grad_(True)
            q(xt).backward(g)
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
        _line("INT kernel, gx + range gradients", tk, 12.0 * n)
        _line("INT kernel, range gradients only", t8, 8.0 * n)
        _line("FP kernel (E5M2), gx + gmaxval", tfp, 12.0 * n, f"   INT / FP time {tk / tfp:5.2f}")
        _line("forward + backward, kernel route", tk_fb, None, f"   peak memory {peak_k / 1e6:9.2f} MB   "
                                                                f"{tc_fb / tk_fb:5.2f}x faster than the torch chain")
        _line("forward + backward, torch chain", tc_fb, None, f"   peak memory {peak_c / 1e6:9.2f} MB")
        worst = tc_fb / tk_fb if worst is None else min(worst, tc_fb / tk_fb)
        del x, g
        torch.cuda.empty_cache()
    print(f"smallest speed-up of forward + backward on the kernel route over the torch chain: {worst:4.2f}x")
    return 0


if __name__ == "__main__":
    sys.exit(main())
