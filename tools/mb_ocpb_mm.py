#!/usr/bin/env python
"""Micro-benchmark of ops.ocp_block_matmul (csrc/fp8q_ocp_block_mm.hip): [8192, 8192, 8192] and [4096, 4096, 4096], E4M3FN x
E4M3FN, tiles (1, 128) x (128, 128) (the forward product) and (1, 128) x (1, 128) (the dW form).  Per shape, timed next to each
other:
  (p) ocp_block_matmul on the block-scaled operands, once per tile pair;
  (a) mx_matmul E4M3FN x E4M3FN on MX operands of the same tensors: the same panels and instruction with the scales inside it,
      so (p) / (a) is the cost of the promotion;
  (b) the composition (p) replaces: two ocp_block_decode(..., out_dtype=bfloat16) and torch.matmul;
  (c) torch.matmul on operands that are already decoded to bfloat16 -- the yardstick, which this work leaves as it was.
The candidates are interleaved: five rounds, each timing every candidate once as the time per call of `reps` back-to-back calls
between two HIP events (after a warm-up); `reps` is chosen per candidate so that a timed window lasts about 100 ms.  The largest round-to-round spread (max / min) of the (c) calls is printed per shape:
a ratio within that spread of 1 is no difference.  (p) is also given as FLOP/s from 2 M N K over the CALL time (launch included; not a kernel time from a
trace) and as that rate over the dense FP8 matrix peak (256 CUs x 4 SIMDs x 2.4 GHz x one 16x16x128 instruction per 32 cycles:
5.0 PFLOP/s).  Needs a GPU; there is no
CPU path.

    python tools/mb_ocpb_mm.py [--quick] [--shape 8192 4096] [--out profiles/ocpb_mm_mb.txt]
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
ROW, SQ = (1, 128), (128, 128)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocpb_mm_mb.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"y = A . B^T, e4m3fn x e4m3fn; {ROUNDS} interleaved rounds, time per call over windows of about {WINDOW * 1e3:.0f} ms of back-to-back calls, medians in us.  "
        f"(p) ocp_block_matmul, float32 out; (a) mx_matmul; (b) 2 x ocp_block_decode to bfloat16 + torch.matmul; (c) torch.matmul "
        f"on decoded bfloat16")
    for n in a.shape:
        x, w = torch.randn((n, n), device="cuda"), torch.randn((n, n), device="cuda")
        xo, mx_ops = ops.ocp_block_encode(x, E4M3, ROW), tuple(ops.mx_encode(x, E4M3)) + tuple(ops.mx_encode(w, E4M3))
        cands = [("mx", "a", lambda o=mx_ops: ops.mx_matmul(*o))]
        for name, tb in (("1x128 . 128x128", SQ), ("1x128 . 1x128", ROW)):
            wo = ops.ocp_block_encode(w, E4M3, tb)
            da, db = ops.ocp_block_decode(*xo, ROW, torch.bfloat16), ops.ocp_block_decode(*wo, tb, torch.bfloat16)
            cands += [(name, "p", lambda o=(*xo, *wo, ROW, tb): ops.ocp_block_matmul(*o)),
                      (name, "b", lambda o=(xo, wo, tb): torch.matmul(ops.ocp_block_decode(*o[0], ROW, torch.bfloat16),
                                                                      ops.ocp_block_decode(*o[1], o[2], torch.bfloat16).t())),
                      (name, "c", lambda o=(da, db): torch.matmul(o[0], o[1].t()))]
        times = {(c[0], c[1]): [] for c in cands}
        reps = {(c[0], c[1]): _reps(c[2], a.quick) for c in cands}
        for _ in range(ROUNDS):
            for name, kind, fn in cands:
                times[(name, kind)].append(_per_call(fn, reps[(name, kind)]))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        spread = max(max(t) / min(t) for (_, kind), t in times.items() if kind == "c")
        ta = med[("mx", "a")]
        say(f"[{n}, {n}, {n}]:   (a) mx_matmul {ta * 1e6:9.1f}")
        for name in ("1x128 . 128x128", "1x128 . 1x128"):
            tp, tb_, tc = (med[(name, k)] for k in "pbc")
            rate = 2.0 * n ** 3 / tp
            say(f"  {name:16s} (p) {tp * 1e6:9.1f}  (b) {tb_ * 1e6:9.1f}  (c) {tc * 1e6:9.1f}   (p)/(a) {tp / ta:6.3f}  (p)/(b) "
                f"{tp / tb_:6.3f}  (p)/(c) {tp / tc:6.3f}   (p): {rate * 1e-12:7.1f} TFLOP/s by call time, {100.0 * rate / PEAK:5.2f} % of the FP8 peak")
        say(f"  round-to-round spread of the (c) calls (max / min): {spread:5.3f}")
        del cands, x, w, xo, mx_ops
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
