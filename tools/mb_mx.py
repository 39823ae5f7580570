#!/usr/bin/env python
"""Micro-benchmark of the microscaling lane (csrc/fp8q_mx.hip) next to its yardstick, the per-tensor hardware FP8 kernels
(csrc/fp8q_ocp.hip), on the same tensors and in the same process: [8192, 8192] and [4096, 4096], float32 and bfloat16.

  ocp_encode / ocp_decode / ocp_quantize       fp8q_ocp_*, E4M3FN, one scale per tensor                      the yardsticks
  minmax + ocp_encode                          what a user composes today for dynamic scaling: two passes over x
  mx_encode / mx_decode / mx_quantize          fp8q_mx_*, E4M3FN and E2M1, floor; the range found in the same pass
  the same three for e2m3 / e3m2               the 6-bit formats, four codes in three bytes; their yardstick is the MXFP8 row
                                               of the same call on the same tensor (MXFP6 moves fewer bytes than MXFP8)

Algorithmic bytes per element (v = 4 for float32, 2 for bfloat16): FP8 encode / decode v + 1 (+ 1/32 with block scales),
FP6 encode / decode v + 3/4 + 1/32, FP4 encode / decode v + 1/2 + 1/32, quantize 2v, minmax + encode 2v + 1.  The aim of an MX kernel is its OCP twin's time
scaled by the ratio of their bytes, which the last column states next to the measured ratio.

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per candidate the three rounds' times, their median, TB/s over the
algorithmic bytes and that as a fraction of 8 TB/s; per tensor the largest round-to-round spread (max / min) of the OCP
yardsticks, which is what the ratios are to be read against.

    python tools/mb_mx.py [--quick] [--out profiles/mx_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

SHAPES = [(8192, 8192), (4096, 4096)]
ROUNDS = 3
PEAK = 8e12
FP6 = ("e2m3", "e3m2")


def _per_call(fn, reps):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"MX (block 32, E8M0 scales, floor) against per-tensor OCP E4M3FN; {ROUNDS} interleaved rounds, time per call of {reps} "
        f"back-to-back calls; TB/s over the algorithmic bytes, and as a fraction of {PEAK / 1e12:.0f} TB/s")
    e4, e2 = torch.float8_e4m3fn, torch.float4_e2m1fn_x2
    for shape in SHAPES:
        for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
            n = shape[0] * shape[1]
            x = torch.randn(shape, device="cuda").to(dtype)
            mv = x.float().abs().amax().reshape(1)
            scale = ops.ocp_scale(mv, e4)
            y = torch.empty_like(x)
            c8 = torch.empty(shape, dtype=torch.uint8, device="cuda")
            c4 = torch.empty((shape[0], shape[1] // 2), dtype=torch.uint8, device="cuda")
            c6 = {f: torch.empty((shape[0], 3 * shape[1] // 4), dtype=torch.uint8, device="cuda") for f in FP6}
            s6 = {f: torch.empty((shape[0], shape[1] // 32), dtype=torch.uint8, device="cuda") for f in FP6}
            for f in FP6:
                ops.mx_encode(x, f, out=c6[f], scales_out=s6[f])
            sc = torch.empty((shape[0], shape[1] // 32), dtype=torch.uint8, device="cuda")
            ops.mx_encode(x, e4, out=c8, scales_out=sc)            # decode's inputs are real operands
            ops.mx_encode(x, e2, out=c4, scales_out=sc)
            s8 = sc.clone()
            ops.mx_encode(x, e4, out=c8, scales_out=s8)
            b32 = 1.0 / 32

            def minmax_encode():
                m = ops.minmax(x, False, want_maxval=True)[2]
                ops.ocp_encode(x, m, e4, out=c8, want_scale=False)

            cands = [("ocp_encode e4m3fn", v + 1, None, lambda: ops.ocp_encode(x, mv, e4, out=c8, want_scale=False)),
                     ("ocp_decode e4m3fn", v + 1, None, lambda: ops.ocp_decode(c8, scale, out=y, fmt=e4)),
                     ("ocp_quantize e4m3fn", 2 * v, None, lambda: ops.ocp_quantize(x, mv, e4, out=y)),
                     ("minmax + ocp_encode", 2 * v + 1, None, minmax_encode),
                     ("mx_encode e4m3fn", v + 1 + b32, "ocp_encode e4m3fn", lambda: ops.mx_encode(x, e4, out=c8, scales_out=s8)),
                     ("mx_decode e4m3fn", v + 1 + b32, "ocp_decode e4m3fn", lambda: ops.mx_decode(c8, s8, fmt=e4, out=y)),
                     ("mx_quantize e4m3fn", 2 * v, "ocp_quantize e4m3fn", lambda: ops.mx_quantize(x, e4, out=y)),
                     ("mx_encode e2m1", v + 0.5 + b32, "ocp_encode e4m3fn", lambda: ops.mx_encode(x, e2, out=c4, scales_out=sc)),
                     ("mx_decode e2m1", v + 0.5 + b32, "ocp_decode e4m3fn", lambda: ops.mx_decode(c4, sc, fmt=e2, out=y)),
                     ("mx_quantize e2m1", 2 * v, "ocp_quantize e4m3fn", lambda: ops.mx_quantize(x, e2, out=y))]
            for f in FP6:
                cands += [(f"mx_encode {f}", v + 0.75 + b32, "mx_encode e4m3fn",
                           lambda f=f: ops.mx_encode(x, f, out=c6[f], scales_out=s6[f])),
                          (f"mx_decode {f}", v + 0.75 + b32, "mx_decode e4m3fn", lambda f=f: ops.mx_decode(c6[f], s6[f], fmt=f, out=y)),
                          (f"mx_quantize {f}", 2 * v, "mx_quantize e4m3fn", lambda f=f: ops.mx_quantize(x, f, out=y))]
            # the order of the timed loop: decode candidates read what the encode candidates of their own format wrote
            order = [0, 1, 2, 3, 7, 8, 9, 4, 5, 6] + list(range(10, len(cands)))
            times = {name: [] for name, _, _, _ in cands}
            for _ in range(ROUNDS):
                for i in order:
                    name, _, _, fn = cands[i]
                    times[name].append(_per_call(fn, reps))
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            nbytes = {name: b for name, b, _, _ in cands}
            say(f"{list(shape)} {str(dtype).replace('torch.', '')}:")
            for name, b, twin, _ in cands:
                t = med[name]
                rounds = " ".join(f"{u * 1e6:8.1f}" for u in times[name])
                rate = b * n / t
                extra = f"   {t / med[twin]:5.3f} x {twin} (bytes {b / nbytes[twin]:5.3f})" if twin else ""
                say(f"  {name:26s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak{extra}")
            spread = max(max(times[k]) / min(times[k]) for k, _, twin, _ in cands if twin is None)
            say(f"  round-to-round spread of the yardsticks (max / min): {spread:5.3f}")
            del x, y, c8, c4, sc, s8, c6, s6
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
