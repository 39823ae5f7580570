#!/usr/bin/env python
"""Micro-benchmark of the INT quantizers' integer codes (csrc/fp8q_intcodec.hip) next to the kernels they sit beside, on the
same tensors and in the same process: the weight-like [2^21, 3, 7, 7] per channel (symmetric, 8 bit) and the activation
[64, 64, 112, 112] per tensor (asymmetric, 8 bit):

  int_quantize     fp8q_int_quantize_f32      8 B / element (x in, y out)
  int_to_integer   fp8q_int_to_integer_f32    8
  int_encode       fp8q_int_encode            5 (x in, 1-byte codes out)
  int_decode       fp8q_int_decode            5
  FP8 encode       fp8q_encode_u8 (E4M3)      5
  FP8 decode       fp8q_decode_u8 (E4M3)      5

Time per call by HIP events (median of 20 after a warm-up), TB/s over the algorithmic bytes, and every INT time as a ratio to
int_quantize's.  Encode reads what int_quantize reads and writes a quarter of what it writes.

    python tools/mb_int_codes.py [--quick] [--out profiles/int_codes_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

from mb_grad import _events  # noqa: E402

CASES = [((1 << 21, 3, 7, 7), True), ((64, 64, 112, 112), False)]


def main():
    from fp8q import ops
    from quantization.uniform import AsymmetricUniformQuantizer, SymmetricUniformQuantizer
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int_codes_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"INT8 / E4M3, fixed ranges from the tensor's min / max; median of {reps} by HIP events; TB/s over the algorithmic bytes")
    worst = None
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
        say(f"{list(shape)} {'per channel, symmetric' if pc else 'per tensor, asymmetric'}:")
        t_q = _events(lambda: ops.int_quantize(x, *r, out=y), reps)
        t_i = _events(lambda: ops.int_to_integer(x, *r, out=y), reps)
        t_e = _events(lambda: ops.int_encode(x, *r, out=codes), reps)
        t_d = _events(lambda: ops.int_decode(codes, *r, out=y), reps)
        f_e = _events(lambda: ops.encode(x, mv, 3.0, 8, 1, out=codes), reps)
        f_d = _events(lambda: ops.decode(codes, mv, 3.0, 8, 1, out=y), reps)
        for name, t, b, ratio in (("int_quantize", t_q, 8, None), ("int_to_integer", t_i, 8, t_i / t_q),
                                  ("int_encode", t_e, 5, t_e / t_q), ("int_decode", t_d, 5, t_d / t_q),
                                  ("FP8 encode (E4M3)", f_e, 5, None), ("FP8 decode (E4M3)", f_d, 5, None)):
            extra = f"   {ratio:5.2f} x int_quantize's time" if ratio is not None else ""
            say(f"  {name:20s} {t * 1e6:9.1f} us  {b * n / t / 1e12:6.3f} TB/s{extra}")
        worst = t_e / t_q if worst is None else max(worst, t_e / t_q)
        del x, y, codes
        torch.cuda.empty_cache()
    say(f"largest int_encode / int_quantize time ratio: {worst:4.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
