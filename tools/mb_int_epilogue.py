#!/usr/bin/env python
"""Micro-benchmark of the INT fused epilogue (csrc/fp8q_intepilogue.hip): INT8 with a symmetric unsigned and an asymmetric
range, fixed ranges, on three activation tensors of a batch-64 ResNet-18 / MobileNetV2 and the epilogue each of them has:

  [64, 64, 112, 112]   BN + ReLU               (the nontemporal staged kernel)
  [64, 64, 56, 56]     BN + residual + ReLU    (the one-group-per-lane kernel)
  [64, 160, 7, 7]      BN + ReLU6              (the same, latency-bound)

Four candidates per tensor, all in one process and timed interleaved, round-robin:

  fused          ops.int_affine_act_quantize                               8 B / element (12 with a residual)
  two launches   ops.affine_act + ops.int_quantize                         16 (20)
  today's chain  F.batch_norm, (+= residual,) activation, ops.int_quantize  24 (36: the add is a pass of its own)
  FP8 epilogue   ops.affine_act_quantize, E4M3, prepared quantizer          8 (12)

Time per call by HIP events around `--inner` calls (default: enough for a window of about a millisecond), median of
`--reps` windows; the whole table is measured `--rounds` times in the same process and every round is printed, so that the
spread of repeated runs stands next to each difference.  GB/s over the algorithmic bytes of the FUSED form.  There is no
target rate: the file reports what was measured, faster or slower.

    python tools/mb_int_epilogue.py [--quick] [--out profiles/int_epilogue_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM = 8.0e12
CASES = [((64, 64, 112, 112), False, 1, "BN + ReLU"), ((64, 64, 56, 56), True, 1, "BN + residual + ReLU"),
         ((64, 160, 7, 7), False, 2, "BN + ReLU6")]
NAMES = ("fused", "two launches", "today's chain", "FP8 epilogue")


def _window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def _round_robin(fns, reps, inner):
    """median time per call of each candidate, the candidates timed alternately"""
    for f in fns:
        for _ in range(3):
            f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t[i].append(_window(f, inner))
    return [sorted(v)[len(v) // 2] for v in t]


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int_epilogue_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else a.reps
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(torch.cuda.get_device_name(0))
    emit(f"INT8 fused epilogue, fixed ranges; time per call by HIP events, median of {reps} windows, candidates interleaved; "
         f"{a.rounds} rounds in one process")
    verdict = []
    for shape, use_res, act, what in CASES:
        N, C = shape[0], shape[1]
        n = 1
        for s in shape:
            n *= s
        inner = a.inner or max(1, min(200, int(1e-3 / (n * 12 / 4e12 + 4e-6))))
        torch.manual_seed(0)
        x = torch.randn(shape, device="cuda") * 2
        res = torch.randn(shape, device="cuda") if use_res else None
        mean, var = torch.randn(C, device="cuda"), torch.rand(C, device="cuda") + 0.5
        gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
        ab = ops.bn_fold((mean, 1 / torch.sqrt(var + 1e-5), gamma, beta))
        t = ops.affine_act(x, ab, res, act)
        lo, hi = t.amin().reshape(1), t.amax().reshape(1)
        mv = torch.maximum(lo.abs(), hi)
        prep = ops.quantizer_prepare(mv, 3.0, 8, 1)
        y, tmp = torch.empty_like(x), torch.empty_like(x)
        nbytes = (12.0 if use_res else 8.0) * n

        def chain(d, z, sg, sym):
            o = F.batch_norm(x, mean, var, gamma, beta, False, 0.1, 1e-5)
            if use_res:
                o += res
            o = F.relu(o) if act == 1 else F.relu6(o)
            return ops.int_quantize(o, d, z, sg, 8, sym, 1e-8, out=y)

        for sym, qname, xmin in ((True, "symmetric unsigned", torch.zeros_like(lo)), (False, "asymmetric", lo)):
            d, z, sg = ops.int_set_range(xmin, hi, 8, sym)
            fns = [lambda: ops.int_affine_act_quantize(x, d, z, sg, 8, sym, 1e-8, bn_ab=ab, residual=res, act=act, out=y),
                   lambda: ops.int_quantize(ops.affine_act(x, ab, res, act, out=tmp), d, z, sg, 8, sym, 1e-8, out=y),
                   lambda: chain(d, z, sg, sym),
                   lambda: ops.affine_act_quantize(x, mv, 3.0, 8, 1, bn_ab=ab, residual=res, act=act, out=y, prep=prep)]
            emit(f"{list(shape)}, {what}, INT8 {qname} ({inner} calls per window):")
            rounds = [_round_robin(fns, reps, inner) for _ in range(a.rounds)]
            for i, name in enumerate(NAMES):
                ts = [r[i] for r in rounds]
                best = min(ts)
                emit(f"  {name:14s} " + " ".join(f"{v * 1e6:8.2f}" for v in ts) + f" us   best {nbytes / best / 1e9:7.1f} GB/s "
                     f"{nbytes / best / HBM:5.3f} of 8 TB/s" + ("" if i == 0 else f"   {best / min(r[0] for r in rounds):4.2f}x fused"))
            fused = [r[0] for r in rounds]
            spread = (max(fused) - min(fused)) / min(fused)
            two = min(r[1] / r[0] for r in rounds)       # the least favourable round
            fp8 = min(r[3] / r[0] for r in rounds)
            emit(f"  spread of the fused launch over the rounds: {spread * 100:.1f} %;  two launches / fused >= {two:4.2f};  "
                 f"FP8 epilogue / fused >= {fp8:4.2f}")
            verdict.append((two >= 1.0, fp8 >= 1.0 - spread))
    emit("fused not slower than the two launches in every round: " + ("yes" if all(v[0] for v in verdict) else "NO") +
         ";  not slower than the FP8 epilogue beyond its own spread: " + ("yes" if all(v[1] for v in verdict) else "NO"))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
