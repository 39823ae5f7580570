#!/usr/bin/env python
"""Micro-benchmark of the hardware FP8 lanes' stochastic rounding (seed= on the OCP ops: the fp8q_ocpsr_* / fp8q_ocpbsr_* /
fp8q_ocpbtsr_* entries) against the round-to-nearest-even call of the same op, on the same tensor and in the same process:
[8192, 8192], float32 and bfloat16; E4M3FN and E5M2; ocp_encode and ocp_quantize per channel, ocp_block_encode and
ocp_block_quantize under each of the three tiles, ocp_block_encode_t and ocp_block_encode_both under each of their two.

The traffic of an op does not change with the rounding, so the ratio SR / RNE is what the draws (one Philox4x32-10 call per
8 elements where a lane holds 16 consecutive ones -- ocp_encode -- and per 4 elements elsewhere, half of each call unused),
the IEEE division of every element (the RNE kernels multiply by a reciprocal and divide about one dword in 2^14) and the
pre-rounding step cost on top of a pass that HBM bounds.  No ratio is promised: the yardstick is the RNE kernel, which this work
leaves as it was, and the ratios measured are what the README states.

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per tensor the largest round-to-round spread (max / min) of the RNE calls is
printed: a ratio within that spread of 1 is no difference.

    python tools/mb_ocp_sr.py [--quick] [--out profiles/ocp_sr_mb.txt]
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
TILES = ((1, 128), (128, 1), (128, 128))
T_TILES = ((1, 128), (128, 128))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocp_sr_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"hardware FP8 operands, stochastic rounding against round to nearest even of the same op; {ROUNDS} interleaved rounds, "
        f"time per call of {reps} back-to-back calls; TB/s over the algorithmic bytes (scales left out), and as a fraction of "
        f"{PEAK / 1e12:.0f} TB/s")
    R, K = SHAPE
    n = R * K
    for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
        x = torch.randn(SHAPE, device="cuda").to(dtype)
        y = torch.empty_like(x)
        mv = x.float().abs().amax(1)
        co = torch.empty(SHAPE, dtype=torch.uint8, device="cuda")
        ct = torch.empty((K, R), dtype=torch.uint8, device="cuda")
        cands = []          # (name, bytes per element, the RNE call it is measured against, fn)
        for name, fmt in (("e4m3fn", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)):
            ops_ = [("ocp_encode", v + 1, lambda kw, fmt=fmt: ops.ocp_encode(x, mv, fmt, out=co, **kw)),
                    ("ocp_quantize", 2 * v, lambda kw, fmt=fmt: ops.ocp_quantize(x, mv, fmt, out=y, **kw))]
            for t in TILES:
                tn = f"{t[0]}x{t[1]}"
                ops_.append((f"ocp_block_encode {tn}", v + 1, lambda kw, fmt=fmt, t=t: ops.ocp_block_encode(x, fmt, t, out=co, **kw)))
                ops_.append((f"ocp_block_quantize {tn}", 2 * v,
                             lambda kw, fmt=fmt, t=t: ops.ocp_block_quantize(x, fmt, t, out=y, **kw)))
            for t in T_TILES:
                tn = f"{t[0]}x{t[1]}"
                ops_.append((f"ocp_block_encode_t {tn}", v + 1,
                             lambda kw, fmt=fmt, t=t: ops.ocp_block_encode_t(x, fmt, t, out=ct, **kw)))
                ops_.append((f"ocp_block_encode_both {tn}", v + 2,
                             lambda kw, fmt=fmt, t=t: ops.ocp_block_encode_both(x, fmt, t, out=co, out_t=ct, **kw)))
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
            say(f"  {name:42s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak{extra}")
        say(f"  round-to-round spread of the RNE calls (max / min): {spread:5.3f}")
        del x, y, cands
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
