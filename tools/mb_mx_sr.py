#!/usr/bin/env python
"""Micro-benchmark of the microscaling lane's stochastic rounding (seed= on the MX ops: the fp8q_mxsr_* entries) against the
round-to-nearest-even call of the same op, on the same tensor and in the same process: [8192, 8192], float32 and bfloat16;
E4M3FN, E2M1 and e2m3; mx_encode, mx_quantize, mx_encode_t and mx_encode_both (mx_quantize for the two formats torch can hold).

The traffic of an op does not change with the rounding, so the ratio SR / RNE is what the draws (one Philox4x32-10 call per
8 elements where a lane holds 8 consecutive ones -- mx_encode -- and per 4 elements elsewhere, half of each call unused) and
the pre-rounding step cost on top of a pass that HBM bounds.  No ratio is promised: the yardstick is the RNE kernel, which
this work leaves as it was, and the ratios measured are what the README states.

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per tensor the largest round-to-round spread (max / min) of the RNE calls is
printed: a ratio within that spread of 1 is no difference.

    python tools/mb_mx_sr.py [--quick] [--out profiles/mx_sr_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

SHAPE = (8192, 8192)
ROUNDS = 3
PEAK = 8e12
SEED = 0x0123456789ABCDEF


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_sr_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"MX operands (floor), stochastic rounding against round to nearest even of the same op; {ROUNDS} interleaved rounds, time "
        f"per call of {reps} back-to-back calls; TB/s over the algorithmic bytes, and as a fraction of {PEAK / 1e12:.0f} TB/s")
    fmts = [("e4m3fn", torch.float8_e4m3fn, 1.0, True), ("e2m1", torch.float4_e2m1fn_x2, 0.5, True), ("e2m3", "e2m3", 0.75, False)]
    b32 = 1.0 / 32
    R, K = SHAPE
    n = R * K
    for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
        x = torch.randn(SHAPE, device="cuda").to(dtype)
        y = torch.empty_like(x)
        cands = []          # (name, bytes per element, the RNE call it is measured against, fn)
        for name, fmt, c, with_quantize in fmts:
            co = torch.empty((R, int(K * c)), dtype=torch.uint8, device="cuda")
            so = torch.empty((R, K // 32), dtype=torch.uint8, device="cuda")
            ct = torch.empty((K, int(R * c)), dtype=torch.uint8, device="cuda")
            st = torch.empty((K, R // 32), dtype=torch.uint8, device="cuda")
            ops_ = [("mx_encode", v + c + b32, lambda kw, fmt=fmt, co=co, so=so: ops.mx_encode(x, fmt, out=co, scales_out=so, **kw)),
                    ("mx_encode_t", v + c + b32,
                     lambda kw, fmt=fmt, ct=ct, st=st: ops.mx_encode_t(x, fmt, out=ct, scales_out=st, **kw)),
                    ("mx_encode_both", v + 2 * c + 2 * b32,
                     lambda kw, fmt=fmt, co=co, so=so, ct=ct, st=st: ops.mx_encode_both(x, fmt, out=co, scales_out=so, out_t=ct,
                                                                                        scales_out_t=st, **kw))]
            if with_quantize:
                ops_.insert(1, ("mx_quantize", 2 * v, lambda kw, fmt=fmt: ops.mx_quantize(x, fmt, out=y, **kw)))
            for op, b, fn in ops_:
                cands.append((f"{op} {name}", b, None, lambda fn=fn: fn({})))
                cands.append((f"{op} {name} seed=", b, f"{op} {name}", lambda fn=fn: fn({"seed": SEED})))
        times = {c[0]: [] for c in cands}
        for _ in range(ROUNDS):
            for name, _, _, fn in cands:
                times[name].append(_per_call(fn, reps))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        spread = max(max(times[c[0]]) / min(times[c[0]]) for c in cands if c[2] is None)
        say(f"{list(SHAPE)} {str(dtype).replace('torch.', '')}:")
        for name, b, yard, _ in cands:
            t = med[name]
            rounds = " ".join(f"{u * 1e6:8.1f}" for u in times[name])
            rate = b * n / t
            extra = f"   SR / RNE {t / med[yard]:5.3f}" if yard else ""
            say(f"  {name:28s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak{extra}")
        say(f"  round-to-round spread of the RNE calls (max / min): {spread:5.3f}")
        del x, y, cands
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
