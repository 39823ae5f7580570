#!/usr/bin/env python
"""Micro-benchmark of ops.mx_matmul (csrc/fp8q_mx_mm.hip): [8192, 8192, 8192] and [4096, 4096, 4096]; E4M3FN x E4M3FN,
E2M1 x E2M1 and E4M3FN x E2M1.  Per shape and pair, timed next to each other:
  (a) mx_matmul on the MX operands;
  (b) the composition it replaces: two mx_decode(..., out_dtype=bfloat16) and torch.matmul;
  (c) torch.matmul on operands that are already decoded to bfloat16 -- the yardstick, which this work leaves as it was;
  (d) torch._scaled_mm with E8M0 block scales, where the installed torch takes it on this device (tried once, at the end).
The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back calls
between two HIP events (after a warm-up).  The largest round-to-round spread (max / min) of the (c) calls is printed per shape:
a ratio within that spread of 1 is no difference.  (a) is also given as FLOP/s from 2 M N K and as a share of the format's dense
matrix peak (256 CUs x 4 SIMDs x 2.4 GHz x one 16x16x128 instruction per 32 cycles for FP8, per 16 for FP4: 5.0 / 10.1 PFLOP/s;
a mixed pair runs at the wider operand's rate).  Needs a GPU; there is no CPU path.

    python tools/mb_mx_mm.py [--quick] [--shape 8192 4096] [--out profiles/mx_mm_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

ROUNDS = 3
E4M3, E2M1 = torch.float8_e4m3fn, torch.float4_e2m1fn_x2
PAIRS = [("e4m3fn x e4m3fn", E4M3, E4M3, 5.03e15), ("e2m1 x e2m1", E2M1, E2M1, 10.07e15), ("e4m3fn x e2m1", E4M3, E2M1, 5.03e15)]


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


def _scaled_mm(n):
    """(d): one attempt; the installed torch's answer is reported as it comes"""
    from fp8q import ops
    x = torch.randn((n, n), device="cuda")
    (ac, asc), (bc, bsc) = ops.mx_encode(x, E4M3), ops.mx_encode(x.t().contiguous(), E4M3)
    try:
        fn = lambda: torch._scaled_mm(ac, bc.t(), scale_a=asc, scale_b=bsc, out_dtype=torch.bfloat16)      # noqa: E731
        t = _per_call(fn, 3)
        return (f"(d) torch._scaled_mm, E8M0 block scales, e4m3fn x e4m3fn [{n}, {n}, {n}]: {t * 1e6:9.1f} us (plain [rows, K / 32] "
                f"scales as given; its result is not compared here)")
    except Exception as exc:        # noqa: BLE001
        return f"(d) torch._scaled_mm with E8M0 block scales: not taken by torch {torch.__version__} on this device: {str(exc)[:160]!r}"


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--shape", type=int, nargs="*", default=[8192, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_mm_mb.txt"))
    a = ap.parse_args()
    reps = 2 if a.quick else 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"y = A . B^T of MX operands; {ROUNDS} interleaved rounds, time per call of {reps} back-to-back calls, medians in us.  "
        f"(a) mx_matmul, float32 out; (b) 2 x mx_decode to bfloat16 + torch.matmul; (c) torch.matmul on decoded bfloat16")
    for n in a.shape:
        x, w = torch.randn((n, n), device="cuda"), torch.randn((n, n), device="cuda")
        cands = []
        for name, fa, fb, peak in PAIRS:
            (ac, asc), (bc, bsc) = ops.mx_encode(x, fa), ops.mx_encode(w, fb)
            da, db = ops.mx_decode(ac, asc, out_dtype=torch.bfloat16), ops.mx_decode(bc, bsc, out_dtype=torch.bfloat16)
            cands += [(name, "a", lambda o=(ac, asc, bc, bsc): ops.mx_matmul(*o)),
                      (name, "b", lambda o=(ac, asc, bc, bsc): torch.matmul(ops.mx_decode(o[0], o[1], out_dtype=torch.bfloat16),
                                                                            ops.mx_decode(o[2], o[3], out_dtype=torch.bfloat16).t())),
                      (name, "c", lambda o=(da, db): torch.matmul(o[0], o[1].t()))]
        times = {(c[0], c[1]): [] for c in cands}
        for _ in range(ROUNDS):
            for name, kind, fn in cands:
                times[(name, kind)].append(_per_call(fn, reps))
        med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
        spread = max(max(t) / min(t) for (_, kind), t in times.items() if kind == "c")
        say(f"[{n}, {n}, {n}]:")
        for name, _, _, peak in PAIRS:
            ta, tb, tc = (med[(name, k)] for k in "abc")
            rate = 2.0 * n ** 3 / ta
            say(f"  {name:18s} (a) {ta * 1e6:9.1f}  (b) {tb * 1e6:9.1f}  (c) {tc * 1e6:9.1f}   (a)/(b) {ta / tb:6.3f}  (a)/(c) {ta / tc:6.3f}   "
                f"(a): {rate * 1e-12:7.1f} TFLOP/s, {100.0 * rate / peak:5.2f} % of the format's peak")
        say(f"  round-to-round spread of the (c) calls (max / min): {spread:5.3f}")
        del cands, x, w
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(a.out, "a") as f:        # (d) last, after everything above is on disk
        d = _scaled_mm(min(a.shape))
        print(d, flush=True)
        f.write(d + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
