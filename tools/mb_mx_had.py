#!/usr/bin/env python
"""Micro-benchmark of the MX lane's block Hadamard rotation (hadamard= on the MX ops: the fp8q_mxh_* entries): [8192, 8192] and
[4096, 4096], float32 and bfloat16; E4M3FN, E2M1 and e2m3; round to nearest even and seed=; mx_encode, mx_quantize and
mx_encode_t.  Each fused call is timed next to
  (a) the same op without a rotation -- the yardstick, which this work leaves as it was;
  (b) the composition it replaces: ops.hadamard32, the op, and for quantize ops.hadamard32(inverse=True) (for mx_encode_t the
      rotation of x.t().contiguous() and mx_encode);
  (c) the rotation as a torch matmul by the signed 32 x 32 matrix in front of the op, which is what a user had before.
The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up).  Per tensor the largest round-to-round spread (max / min) of the (a) calls is
printed: a ratio within that spread of 1 is no difference.

    python tools/mb_mx_had.py [--quick] [--shape 8192] [--out profiles/mx_had_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

ROUNDS = 3
SEED = 0x0123456789ABCDEF
MASK = 0x9E3779B9


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
    ap.add_argument("--shape", type=int, nargs="*", default=[8192, 4096])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_had_mb.txt"))
    a = ap.parse_args()
    reps = 3 if a.quick else 10
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"MX operands (floor) under a block Hadamard rotation; {ROUNDS} interleaved rounds, time per call of {reps} back-to-back "
        f"calls, medians in us.  fused: hadamard=; (a) no rotation; (b) ops.hadamard32 + op (+ inverse); (c) torch matmul + op")
    i = torch.arange(32)
    sg = torch.tensor([-1.0 if MASK >> k & 1 else 1.0 for k in range(32)])
    H = torch.tensor([[(-1.0) ** bin(int(p & q)).count("1") for q in i] for p in i]) * 2.0 ** -2.5
    fmts = [("e4m3fn", torch.float8_e4m3fn), ("e2m1", torch.float4_e2m1fn_x2), ("e2m3", "e2m3")]
    for n in a.shape:
        for dtype in (torch.float32, torch.bfloat16):
            x = torch.randn((n, n), device="cuda").to(dtype)
            Hs = (sg[:, None] * H).cuda().to(dtype)             # y = x_block @ Hs: the signs, then the transform
            Hi = Hs.t().contiguous()                            # the inverse
            cands = []                                          # (name, kind, fn)
            for fname, fmt in fmts:
                for rname, kw in (("rne", {}), ("sr", {"seed": SEED})):
                    def rot(t, inverse=False, out_dtype=None):
                        return ops.hadamard32(t, MASK, inverse=inverse, out_dtype=out_dtype)

                    def mm(t, M=Hs):
                        return (t.reshape(-1, 32) @ M).view(t.shape)

                    enc = lambda t, h=None, fmt=fmt, kw=kw: ops.mx_encode(t, fmt, hadamard=h, **kw)            # noqa: E731
                    qnt = lambda t, h=None, fmt=fmt, kw=kw, od=None: ops.mx_quantize(t, fmt, hadamard=h, out_dtype=od, **kw)  # noqa: E731
                    enct = lambda t, h=None, fmt=fmt, kw=kw: ops.mx_encode_t(t, fmt, hadamard=h, **kw)         # noqa: E731
                    tag = f"{fname} {rname}"
                    cands += [
                        (f"mx_encode {tag}", "fused", lambda enc=enc: enc(x, MASK)),
                        (f"mx_encode {tag}", "a", lambda enc=enc: enc(x)),
                        (f"mx_encode {tag}", "b", lambda enc=enc, rot=rot: enc(rot(x))),
                        (f"mx_encode {tag}", "c", lambda enc=enc, mm=mm: enc(mm(x))),
                        (f"mx_quantize {tag}", "fused", lambda qnt=qnt: qnt(x, MASK, od=dtype)),
                        (f"mx_quantize {tag}", "a", lambda qnt=qnt: qnt(x, od=dtype)),
                        (f"mx_quantize {tag}", "b", lambda qnt=qnt, rot=rot: rot(qnt(rot(x)), True, dtype)),
                        (f"mx_quantize {tag}", "c", lambda qnt=qnt, mm=mm: mm(qnt(mm(x), od=dtype), Hi)),
                        (f"mx_encode_t {tag}", "fused", lambda enct=enct: enct(x, MASK)),
                        (f"mx_encode_t {tag}", "a", lambda enct=enct: enct(x)),
                        (f"mx_encode_t {tag}", "b", lambda enc=enc, rot=rot: enc(rot(x.t().contiguous()))),
                        (f"mx_encode_t {tag}", "c", lambda enc=enc, mm=mm: enc(mm(x.t().contiguous()))),
                    ]
            times = {(c[0], c[1]): [] for c in cands}
            for _ in range(ROUNDS):
                for name, kind, fn in cands:
                    times[(name, kind)].append(_per_call(fn, reps))
            med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
            spread = max(max(t) / min(t) for (_, kind), t in times.items() if kind == "a")
            say(f"[{n}, {n}] {str(dtype).replace('torch.', '')}:")
            for name in dict.fromkeys(c[0] for c in cands):
                f, ya, yb, yc = (med[(name, k)] for k in ("fused", "a", "b", "c"))
                say(f"  {name:24s} fused {f * 1e6:8.1f}  (a) {ya * 1e6:8.1f}  (b) {yb * 1e6:8.1f}  (c) {yc * 1e6:8.1f}   "
                    f"fused/(a) {f / ya:5.3f}  fused/(b) {f / yb:5.3f}  fused/(c) {f / yc:5.3f}")
            say(f"  round-to-round spread of the (a) calls (max / min): {spread:5.3f}")
            del x, cands
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
