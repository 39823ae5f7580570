#!/usr/bin/env python
"""Micro-benchmark of ops.mx_matmul(skinny=True) (csrc/fp8q_mx_mm_skinny.hip): W of [8192, 8192] and [28672, 8192]; M of 1, 16
and 64; E4M3FN x E4M3FN, E4M3FN x E2M1 and E2M1 x E2M1 (activations x weights).  Per shape and pair, timed next to each other:
  (a) mx_matmul(skinny=True), float32 out, its workspace passed by the caller as a decode loop would;
  (b) mx_matmul(skinny=False): the tiled kernel, the thing to beat;
  (c) mx_decode of W to bfloat16 + torch.matmul;
  (d) torch.matmul on a W that is already decoded to bfloat16 -- the yardstick, whose round-to-round spread is printed.
Every candidate rotates through distinct W tensors whose total exceeds 512 MiB, so that every call reads its W from HBM and not
from the 256 MiB last-level cache a single W of 32-64 MiB would stay in.  The candidates are interleaved: three rounds, each
timing every candidate once as the time per call of `reps` back-to-back calls between two HIP events (after a warm-up).  A
ratio within the printed spread of 1 is no difference.  (a) is also given as bytes per call (W codes + W scales + X codes + X
scales + y, from the shapes) over the CALL time -- launch gaps and, where the plan splits, the reduce launch included; it is not
kernel time -- and as a share of 8 TB/s.  --splits tries forced split counts on (a) for the plan's constants.  Needs a GPU.

    python tools/mb_mx_skinny.py [--quick] [--n 8192 28672] [--m 1 16 64] [--splits 4 16] [--out profiles/mx_skinny_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

ROUNDS, K, HBM = 3, 8192, 8.0e12
E4M3, E2M1 = torch.float8_e4m3fn, torch.float4_e2m1fn_x2
PAIRS = [("e4m3fn x e4m3fn", E4M3, E4M3), ("e4m3fn x e2m1", E4M3, E2M1), ("e2m1 x e2m1", E2M1, E2M1)]


def _per_call(fn, n_w, reps):
    """fn(i) uses W number i % n_w; warm-up and the timed calls walk the ring"""
    for i in range(2):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(i % n_w)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--n", type=int, nargs="*", default=[8192, 28672])
    ap.add_argument("--m", type=int, nargs="*", default=[1, 16, 64])
    ap.add_argument("--splits", type=int, nargs="*", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_skinny_mb.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"y[M, N] = X[M, {K}] . W[N, {K}]^T; {ROUNDS} interleaved rounds, W rotating over > 512 MiB per candidate, medians of the "
        f"time per call in us.  (a) skinny=True  (b) skinny=False  (c) mx_decode(W) to bfloat16 + torch.matmul  (d) torch.matmul "
        f"on decoded bfloat16")
    for n in a.n:
        for name, fx, fw in PAIRS:
            wbytes = n * K * (1 if fw == E4M3 else 0.5) + n * K // 32
            n_w = int(512 * 2 ** 20 // wbytes) + 1      # the (d) copies are bfloat16, four times larger at least
            n_d = int(512 * 2 ** 20 // (n * K * 2)) + 1
            reps = max(n_w, 6) if a.quick else max(2 * n_w, 30)
            ws_ = [ops.mx_encode(torch.randn((n, K), device="cuda"), fw) for _ in range(n_w)]
            wd = [ops.mx_decode(*ws_[i], out_dtype=torch.bfloat16) for i in range(n_d)]
            for m in a.m:
                xc, xs = ops.mx_encode(torch.randn((m, K), device="cuda"), fx)
                xd = ops.mx_decode(xc, xs, out_dtype=torch.bfloat16)
                cands = []
                for sp in [None] + a.splits:
                    plan = ops.mx_skinny_plan(m, n, K, sp)
                    wk = torch.empty(max(plan[3], 16), dtype=torch.uint8, device="cuda")
                    cands.append((f"a{'' if sp is None else sp}", n_w, plan,
                                  lambda i, sp=sp, wk=wk: ops.mx_matmul(xc, xs, *ws_[i], skinny=True, splits=sp, workspace=wk)))
                cands += [("b", n_w, None, lambda i: ops.mx_matmul(xc, xs, *ws_[i])),
                          ("c", n_w, None, lambda i: torch.matmul(xd, ops.mx_decode(*ws_[i], out_dtype=torch.bfloat16).t())),
                          ("d", n_d, None, lambda i: torch.matmul(xd, wd[i].t()))]
                times = {c[0]: [] for c in cands}
                for _ in range(ROUNDS):
                    for kind, ring, _, fn in cands:
                        times[kind].append(_per_call(fn, ring, reps))
                med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
                spread = max(times["d"]) / min(times["d"])
                nbytes = wbytes + xc.numel() + xs.numel() + m * n * 4
                say(f"[M {m:2d}, N {n}, K {K}] {name:16s} (a) {med['a'] * 1e6:7.1f}  (b) {med['b'] * 1e6:7.1f}  (c) {med['c'] * 1e6:7.1f}  "
                    f"(d) {med['d'] * 1e6:7.1f}   (a)/(b) {med['a'] / med['b']:5.3f}  (a)/(c) {med['a'] / med['c']:5.3f}  (a)/(d) "
                    f"{med['a'] / med['d']:5.3f}  spread of (d) {spread:5.3f}   (a): plan (S, T, tw) {cands[0][2][:3]}, "
                    f"{nbytes / 2 ** 20:6.1f} MiB per call, {nbytes / med['a'] * 1e-12:5.2f} TB/s of call time, "
                    f"{100.0 * nbytes / med['a'] / HBM:4.1f} % of 8 TB/s")
                for kind, _, plan, _ in cands[1:1 + len(a.splits)]:
                    say(f"      forced splits {kind[1:]:>4s}: plan (S, T, tw) {plan[:3]}  {med[kind] * 1e6:7.1f} us  "
                        f"{med[kind] / med['a']:5.3f} x the plan's own")
            del ws_, wd
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
