#!/usr/bin/env python
"""Micro-benchmark of the storage codes of half tensors (csrc/fp8q_codec_h16.hip): E5M2 (FP8) and INT8 codes, for bfloat16
and float16, on the weight-shaped tensor [2^21, 3, 7, 7] per channel and the activation-shaped tensor [64, 64, 112, 112] per
tensor, all in one process:

  half -> codes                   fp8q_encode_h16 / fp8q_int_encode_h16                3 B / element
  widen, fp32 encode              ops.encode(x.float(), ...) / ops.int_encode(...)     11  (2+4, 4+1): the only route half
                                  data had before these kernels existed
  codes -> half                   fp8q_decode_h16 / fp8q_int_decode_h16                3
  fp32 decode, narrow             ops.decode(c, ...).to(dtype) / ops.int_decode(...)   11  (1+4, 4+2)

Time per call by HIP events (median of 20 after a warm-up); the half route and the chain it replaces are timed interleaved,
call by call.  GB/s over the algorithmic bytes and the fraction of 8 TB/s; the last column of a half line is its speed-up
over the chain.  There is no target: the file reports what was measured, faster or slower.

    python tools/mb_h16_codes.py [--quick] [--out profiles/h16_codes_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

HBM = 8.0e12
CASES = [((1 << 21, 3, 7, 7), True), ((64, 64, 112, 112), False)]


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def _pair(f, g, reps):
    """medians of f and g, timed alternately"""
    for _ in range(3):
        f()
        g()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(_timed(f))
        tg.append(_timed(g))
    tf.sort()
    tg.sort()
    return tf[len(tf) // 2], tg[len(tg) // 2]


def main():
    from fp8q import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "h16_codes_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def line(name, t, nbytes, extra=""):
        emit(f"  {name:34s} {t * 1e6:9.1f} us  {nbytes / t / 1e9:8.1f} GB/s  {nbytes / t / HBM:5.3f} of 8 TB/s{extra}")

    emit(torch.cuda.get_device_name(0))
    emit(f"storage codes of half tensors, E5M2 and INT8 (asymmetric), fixed ranges; median of {reps} by HIP events, "
         "half route and chain interleaved")
    ratios = []
    for shape, pc in CASES:
        n = 1
        for s in shape:
            n *= s
        x32 = torch.randn(shape, device="cuda")
        C = shape[0] if pc else 1
        lo = x32.view(C, -1).amin(1).contiguous()
        hi = x32.view(C, -1).amax(1).contiguous()
        mv = torch.maximum(lo.abs(), hi)
        d, z, sg = ops.int_set_range(lo, hi, 8, False)
        fams = (("E5M2", lambda t, out: ops.encode(t, mv, 2.0, 8, 1, out=out),
                 lambda c, **kw: ops.decode(c, mv, 2.0, 8, 1, **kw)),
                ("INT8", lambda t, out: ops.int_encode(t, d, z, sg, 8, False, out=out),
                 lambda c, **kw: ops.int_decode(c, d, z, sg, 8, False, **kw)))
        for dt in (torch.bfloat16, torch.float16):
            x = x32.to(dt)
            name = str(dt).replace("torch.", "")
            for fam, enc, dec in fams:
                emit(f"{list(shape)}, {'per channel' if pc else 'per tensor'}, {fam}, {name}:")
                codes = torch.empty(shape, dtype=torch.uint8, device="cuda")
                codes2 = torch.empty_like(codes)
                y = torch.empty_like(x)
                te, tce = _pair(lambda: enc(x, codes), lambda: enc(x.float(), codes2), reps)
                line("half -> codes", te, 3.0 * n, f"   {tce / te:4.2f}x the chain below")
                line("widen, fp32 encode", tce, 11.0 * n)
                td, tcd = _pair(lambda: dec(codes, out=y), lambda: dec(codes).to(dt), reps)
                line("codes -> half", td, 3.0 * n, f"   {tcd / td:4.2f}x the chain below")
                line("fp32 decode, narrow", tcd, 11.0 * n)
                ratios += [tce / te, tcd / td]
                del codes, codes2, y
                torch.cuda.empty_cache()
            del x
        del x32
        torch.cuda.empty_cache()
    emit(f"half route over the chain it replaces: {min(ratios):4.2f}x to {max(ratios):4.2f}x "
         f"({'faster in every case' if min(ratios) > 1 else 'NOT faster in every case'})")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
