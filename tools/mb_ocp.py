#!/usr/bin/env python
"""Micro-benchmark of the hardware FP8 lane (csrc/fp8q_ocp.hip) next to its yardstick, the INT8 quantizer's kernels, which
move the same bytes per element and carry one constant per row as well -- on the same tensors and in the same process: the
weight-like [2^21, 3, 7, 7] per channel and the activation [64, 64, 112, 112] per tensor:

  int_encode / int_decode / int_quantize       fp8q_int_encode / _decode / fp8q_int_quantize_f32, 8 bit    5 / 5 / 8 B per element
  ocp_encode / ocp_decode / ocp_quantize       fp8q_ocp_*_f32, E4M3FN and E5M2                              5 / 5 / 8

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per candidate the three rounds' times, their median, TB/s over the
algorithmic bytes, and for the OCP candidates the ratio of medians to the INT twin; per tensor the largest round-to-round
spread (max / min) of the INT yardsticks, which is what the ratios are to be read against.

    python tools/mb_ocp.py [--quick] [--out profiles/ocp_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

CASES = [((1 << 21, 3, 7, 7), True), ((64, 64, 112, 112), False)]
ROUNDS = 3


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
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocp_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"INT8 against OCP E4M3FN / E5M2, fixed ranges from the tensor's min / max; {ROUNDS} interleaved rounds, time per call of "
        f"{reps} back-to-back calls; TB/s over the algorithmic bytes")
    for shape, pc in CASES:
        n = 1
        for s in shape:
            n *= s
        x = torch.randn(shape, device="cuda")
        q = (SymmetricUniformQuantizer if pc else AsymmetricUniformQuantizer)(n_bits=8, per_channel=pc)
        rows = x.view(shape[0], -1) if pc else x.view(1, -1)
        q.set_quant_range(rows.amin(1).contiguous(), rows.amax(1).contiguous())
        r = (q._delta, None if pc else q._zero_float, q._signed if pc else None, 8, pc, q.eps)
        mv = rows.abs().amax(1).contiguous()
        y = torch.empty_like(x)
        codes = torch.empty(shape, dtype=torch.uint8, device="cuda")
        cands = [("int_encode", 5, None, lambda: ops.int_encode(x, *r, out=codes)),
                 ("int_decode", 5, None, lambda: ops.int_decode(codes, *r, out=y)),
                 ("int_quantize", 8, None, lambda: ops.int_quantize(x, *r, out=y))]
        for fmt, tag in ((torch.float8_e4m3fn, "e4m3fn"), (torch.float8_e5m2, "e5m2")):
            scale = ops.ocp_scale(mv, fmt)
            cands += [(f"ocp_encode {tag}", 5, "int_encode",
                       lambda fmt=fmt: ops.ocp_encode(x, mv, fmt, out=codes, want_scale=False)),
                      (f"ocp_decode {tag}", 5, "int_decode", lambda fmt=fmt, scale=scale: ops.ocp_decode(codes, scale, out=y, fmt=fmt)),
                      (f"ocp_quantize {tag}", 8, "int_quantize", lambda fmt=fmt: ops.ocp_quantize(x, mv, fmt, out=y))]
        times = {name: [] for name, _, _, _ in cands}
        for _ in range(ROUNDS):
            for name, _, _, fn in cands:
                times[name].append(_per_call(fn, reps))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        say(f"{list(shape)} {'per channel' if pc else 'per tensor'}:")
        for name, b, twin, _ in cands:
            t = med[name]
            rounds = " ".join(f"{v * 1e6:8.1f}" for v in times[name])
            extra = f"   {t / med[twin]:5.3f} x {twin}" if twin else ""
            say(f"  {name:20s} rounds {rounds} us  median {t * 1e6:8.1f} us  {b * n / t / 1e12:6.3f} TB/s{extra}")
        spread = max(max(times[k]) / min(times[k]) for k in ("int_encode", "int_decode", "int_quantize"))
        say(f"  round-to-round spread of the INT yardsticks (max / min): {spread:5.3f}")
        del x, y, codes
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
