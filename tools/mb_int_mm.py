#!/usr/bin/env python
"""Micro-benchmark of ops.int_matmul (csrc/fp8q_int_mm.hip): [8192, 8192, 8192] and [4096, 4096, 4096], A asymmetric per tensor
x B symmetric signed per channel, 8 bits both (the W8A8 setting).  Per shape, timed next to each other:
  (a) int_matmul on the codes, float32 out;
  (b) the composition it replaces: two int_decode(..., out_dtype=bfloat16) and torch.matmul;
  (c) torch.matmul on operands that are already decoded to bfloat16 -- the yardstick, which this work leaves as it was;
  (d) the FP8 products at the same shape: mx_matmul E4M3FN x E4M3FN, and ocp_block_matmul E4M3FN x E4M3FN under (1, 128) x
      (128, 128) tiles: the same panels and tile loop around the FP8 instruction.
The candidates are interleaved: five rounds, each timing every candidate once as the time per call of `reps` back-to-back calls
between two HIP events (after a warm-up); `reps` is chosen per candidate so that a timed window lasts about 100 ms.  Each
candidate's own round-to-round spread (max / min of its five rounds) is printed: a ratio within the spreads of 1 is no
difference.  (a) is also given as OP/s from 2 M N K over the CALL time (launch included; not a kernel time from a trace) and
as that rate over the dense INT8 matrix peak of the spec sheet, which equals the FP8 one that tools/mb_ocpb_mm.py uses
(5.0 POP/s; the instruction's own issue rate was not measured).  Needs a GPU; there is no CPU path.

    python tools/mb_int_mm.py [--quick] [--shape 8192 4096] [--out profiles/int_mm_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

ROUNDS = 5
WINDOW = 0.1      # seconds of back-to-back calls per timed window
E4M3 = torch.float8_e4m3fn
BF16 = torch.bfloat16
PEAK = 5.03e15


def _reps(fn, quick):
    """calls that fill a window: from one timed call after a warm-up"""
    return 2 if quick else max(5, int(WINDOW / _per_call(fn, 1)) + 1)


def _per_call(fn, reps):
    for _ in range(2):
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
    ap.add_argument("--shape", type=int, nargs="*", default=[8192, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int_mm_mb.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"y = A . B^T, A asymmetric per tensor x B symmetric signed per channel, 8 bits; {ROUNDS} interleaved rounds, time per call "
        f"over windows of about {WINDOW * 1e3:.0f} ms of back-to-back calls, medians in us, [spread: max / min of the candidate's "
        f"rounds].  (a) int_matmul, float32 out; (b) 2 x int_decode to bfloat16 + torch.matmul; (c) torch.matmul on decoded "
        f"bfloat16; (d) mx_matmul and ocp_block_matmul, e4m3fn x e4m3fn")
    for n in a.shape:
        x, w = torch.randn((n, n), device="cuda"), torch.randn((n, n), device="cuda")
        flag = torch.ones(1, dtype=torch.uint8, device="cuda")
        xq = (x.max() - x.min()).reshape(1) / 255.0, (-x.min()).reshape(1) / ((x.max() - x.min()) / 255.0)    # delta, zero_float
        wd = w.abs().amax(1) / 127.0
        xc, wc = ops.int_encode(x, *xq), ops.int_encode(w, wd, None, flag, 8, True)
        dx, dw = ops.int_decode(xc, *xq, out_dtype=BF16), ops.int_decode(wc, wd, None, flag, 8, True, out_dtype=BF16)
        mx_ops = tuple(ops.mx_encode(x, E4M3)) + tuple(ops.mx_encode(w, E4M3))
        ob_ops = tuple(ops.ocp_block_encode(x, E4M3, (1, 128))) + tuple(ops.ocp_block_encode(w, E4M3, (128, 128)))
        cands = [("a", lambda: ops.int_matmul(xc, xq[0], wc, wd, a_zero_float=xq[1], b_signed_flag=flag, b_symmetric=True)),
                 ("b", lambda: torch.matmul(ops.int_decode(xc, *xq, out_dtype=BF16),
                                            ops.int_decode(wc, wd, None, flag, 8, True, out_dtype=BF16).t())),
                 ("c", lambda: torch.matmul(dx, dw.t())),
                 ("d mx", lambda: ops.mx_matmul(*mx_ops)),
                 ("d ocpb", lambda: ops.ocp_block_matmul(*ob_ops, (1, 128), (128, 128)))]
        y = cands[0][1]()
        ref = (dx.float() @ dw.float().t())
        say(f"[{n}, {n}, {n}]:   largest |int_matmul - product of the bfloat16 decodes| / largest |product|: "
            f"{((y - ref).abs().max() / ref.abs().max()).item():.2e}")
        del y, ref
        times = {c[0]: [] for c in cands}
        reps = {c[0]: _reps(c[1], a.quick) for c in cands}
        for _ in range(ROUNDS):
            for name, fn in cands:
                times[name].append(_per_call(fn, reps[name]))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        say("  " + "   ".join(f"({k}) {med[k] * 1e6:9.1f} [{max(t) / min(t):5.3f}]" for k, t in times.items()))
        ta = med["a"]
        rate = 2.0 * n ** 3 / ta
        say("  " + "  ".join(f"(a)/({k}) {ta / med[k]:6.3f}" for k in list(med)[1:]) +
            f"   (a): {rate * 1e-12:7.1f} TOP/s by call time, {100.0 * rate / PEAK:5.2f} % of the INT8 peak")
        del cands, x, w, xc, wc, dx, dw, mx_ops, ob_ops
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
