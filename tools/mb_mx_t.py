#!/usr/bin/env python
"""Micro-benchmark of the microscaling lane with the blocks along dim 0 (csrc/fp8q_mx_t.hip) next to what it replaces, on the
same tensors and in the same process: [8192, 8192] and [4096, 4096], float32 and bfloat16; E4M3FN and E2M1, plus e2m3 for the
encoders.

  mx_encode                                         row-wise, fp8q_mx_encode_*                                the yardstick
  x.t().contiguous() + mx_encode                    what a user writes today for the transposed operands
  mx_encode_t                                       fp8q_mxt_encode_*: the same bytes from x as it lies
  mx_encode + (x.t().contiguous() + mx_encode)      both orientations today
  mx_encode_both                                    fp8q_mxt_encode_both_*: both from one read of x
  mx_quantize                                       row-wise fake-quantize                                    the yardstick
  mx_quantize(x.t().contiguous()).t().contiguous()  fake-quantize along dim 0 today
  mx_quantize_t                                     fp8q_mxt_quantize_*

Algorithmic bytes per element (v = 4 for float32, 2 for bfloat16; c = 1, 3/4, 1/2 for FP8, FP6, FP4): encode and encode_t
v + c + 1/32, the transposed composition 3v + c + 1/32, both orientations today 4v + 2c + 1/16, encode_both v + 2c + 1/16,
quantize and quantize_t 2v, the quantize composition 6v.  Beside each measured ratio stands the ratio of those bytes.

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per tensor the largest round-to-round spread (max / min) of the yardsticks is
printed.  Acceptance is relative to code that existed before this lane: a new entry's median must lie below the median of the
composition it replaces by more than that spread; each such line ends in PASS or FAIL, and the last line counts them.

    python tools/mb_mx_t.py [--quick] [--out profiles/mx_t_mb.txt]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_t_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"MX operands with the blocks along dim 0 (floor) against the compositions they replace; {ROUNDS} interleaved rounds, time "
        f"per call of {reps} back-to-back calls; TB/s over the algorithmic bytes, and as a fraction of {PEAK / 1e12:.0f} TB/s")
    fmts = [("e4m3fn", torch.float8_e4m3fn, 1.0, True), ("e2m1", torch.float4_e2m1fn_x2, 0.5, True), ("e2m3", "e2m3", 0.75, False)]
    b32 = 1.0 / 32
    passed = failed = 0
    for shape in SHAPES:
        for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
            R, K = shape
            n = R * K
            x = torch.randn(shape, device="cuda").to(dtype)
            y = torch.empty_like(x)
            cands = []          # (name, bytes per element, the composition it replaces, its yardstick, fn)
            for name, fmt, c, with_quantize in fmts:
                kc = int(K * c)
                rc = int(R * c)
                co = torch.empty((R, kc), dtype=torch.uint8, device="cuda")
                so = torch.empty((R, K // 32), dtype=torch.uint8, device="cuda")
                ct = torch.empty((K, rc), dtype=torch.uint8, device="cuda")
                st = torch.empty((K, R // 32), dtype=torch.uint8, device="cuda")

                def enc(fmt=fmt, co=co, so=so):
                    ops.mx_encode(x, fmt, out=co, scales_out=so)

                def comp(fmt=fmt, ct=ct, st=st):
                    ops.mx_encode(x.t().contiguous(), fmt, out=ct, scales_out=st)

                def both_today(enc=enc, comp=comp):
                    enc()
                    comp()

                cands += [(f"mx_encode {name}", v + c + b32, None, None, enc),
                          (f"t().contiguous() + mx_encode {name}", 3 * v + c + b32, None, f"mx_encode {name}", comp),
                          (f"mx_encode_t {name}", v + c + b32, f"t().contiguous() + mx_encode {name}", f"mx_encode {name}",
                           lambda fmt=fmt, ct=ct, st=st: ops.mx_encode_t(x, fmt, out=ct, scales_out=st)),
                          (f"mx_encode + composition {name}", 4 * v + 2 * c + 2 * b32, None, f"mx_encode {name}", both_today),
                          (f"mx_encode_both {name}", v + 2 * c + 2 * b32, f"mx_encode + composition {name}", f"mx_encode {name}",
                           lambda fmt=fmt, co=co, so=so, ct=ct, st=st: ops.mx_encode_both(x, fmt, out=co, scales_out=so, out_t=ct,
                                                                                          scales_out_t=st))]
                if with_quantize:
                    cands += [(f"mx_quantize {name}", 2 * v, None, None, lambda fmt=fmt: ops.mx_quantize(x, fmt, out=y)),
                              (f"mx_quantize(t().contiguous()).t().contiguous() {name}", 6 * v, None, f"mx_quantize {name}",
                               lambda fmt=fmt: ops.mx_quantize(x.t().contiguous(), fmt).t().contiguous()),
                              (f"mx_quantize_t {name}", 2 * v, f"mx_quantize(t().contiguous()).t().contiguous() {name}",
                               f"mx_quantize {name}", lambda fmt=fmt: ops.mx_quantize_t(x, fmt, out=y))]
            times = {c[0]: [] for c in cands}
            for _ in range(ROUNDS):
                for name, _, _, _, fn in cands:
                    times[name].append(_per_call(fn, reps))
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            nbytes = {c[0]: c[1] for c in cands}
            spread = max(max(times[c[0]]) / min(times[c[0]]) for c in cands if c[3] is None)
            say(f"{list(shape)} {str(dtype).replace('torch.', '')}:")
            for name, b, replaces, yard, _ in cands:
                t = med[name]
                rounds = " ".join(f"{u * 1e6:8.1f}" for u in times[name])
                rate = b * n / t
                extra = ""
                if yard:
                    extra += f"   {t / med[yard]:5.3f} x {yard} (bytes {b / nbytes[yard]:5.3f})"
                if replaces:
                    ok = med[replaces] / t > spread
                    passed, failed = passed + ok, failed + (not ok)
                    extra += f"   {t / med[replaces]:5.3f} x the composition (bytes {b / nbytes[replaces]:5.3f})  {'PASS' if ok else 'FAIL'}"
                say(f"  {name:52s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak{extra}")
            say(f"  round-to-round spread of the yardsticks (max / min): {spread:5.3f}")
            del x, y, cands
            torch.cuda.empty_cache()
    say(f"acceptance (a new entry below the composition it replaces by more than the spread): {passed} PASS, {failed} FAIL")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
