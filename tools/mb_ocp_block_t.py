#!/usr/bin/env python
"""Micro-benchmark of the transposed operands of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block_t.hip) next to the
compositions they replace and to their yardsticks, on the same tensor and in the same process: [8192, 8192] and [4096, 4096],
float32 and bfloat16, E4M3FN, tiles 1x128 and 128x128.

  ocp_encode (per tensor, the range given), ocp_block_encode      the yardsticks: the row-wise kernels
  x.t().contiguous() + ocp_block_encode                           encode_t today: a transposed copy, then one pass over it
  that composition + ocp_block_encode(x)                          encode_both today
  ocp_block_encode_t / ocp_block_encode_both                      one pass over x as it lies

Algorithmic bytes per element (v = 4 for float32, 2 for bfloat16; the scale tables add 4 / 128 or 4 / 16384 per orientation):
encode_t v + 1 against 3v + 1 (the copy reads and writes v), encode_both v + 2 against 4v + 2 -- 5 of 13 and 6 of 18 for
float32.

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up); medians are reported, and the largest round-to-round spread (max / min) of the
yardsticks.  No ratio is fixed in advance: each comparison says whether the new call lies below its composition by more than
that spread (BELOW) or does not (NOT BELOW), and the last line counts them.  The ratio to the row-wise ocp_block_encode is
reported beside it and promised nowhere.

    python tools/mb_ocp_block_t.py [--quick] [--out profiles/ocp_block_t_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

SHAPES = ((8192, 8192), (4096, 4096))
ROUNDS = 3
PEAK = 8e12
TILES = ((1, 128), (128, 128))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocp_block_t_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = torch.float8_e4m3fn
    say(torch.cuda.get_device_name(0))
    say(f"transposed tile-scaled OCP E4M3FN against the compositions it replaces and the row-wise kernels; {ROUNDS} interleaved "
        f"rounds, time per call of {reps} back-to-back calls; TB/s over the algorithmic bytes, and as a fraction of "
        f"{PEAK / 1e12:.0f} TB/s")
    below = not_below = 0
    for shape in SHAPES:
        R, K = shape
        n = R * K
        for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
            x = torch.randn(shape, device="cuda").to(dtype)
            co = torch.empty(shape, dtype=torch.uint8, device="cuda")
            cot = torch.empty((K, R), dtype=torch.uint8, device="cuda")
            mv1 = x.float().abs().amax().reshape(1)
            cands = [("ocp_encode per tensor", v + 1, None, None, lambda: ops.ocp_encode(x, mv1, fmt, out=co))]
            for tile in TILES:
                name = f"{tile[0]}x{tile[1]}"
                _, _, sshape, stshape = ops._ocpbt_geometry(x, tile)
                so = torch.empty(sshape, dtype=torch.float32, device="cuda")
                sot = torch.empty(stshape, dtype=torch.float32, device="cuda")
                sb = 4.0 * so.numel() / n
                row = f"ocp_block_encode {name}"

                def comp_t(tile=tile, sot=sot):
                    ops.ocp_block_encode(x.t().contiguous(), fmt, tile, out=cot, scales_out=sot)

                def comp_both(tile=tile, so=so, sot=sot):
                    ops.ocp_block_encode(x.t().contiguous(), fmt, tile, out=cot, scales_out=sot)
                    ops.ocp_block_encode(x, fmt, tile, out=co, scales_out=so)

                cands += [(row, v + 1 + sb, None, None,
                           lambda tile=tile, so=so: ops.ocp_block_encode(x, fmt, tile, out=co, scales_out=so)),
                          (f"composition encode_t {name}", 3 * v + 1 + sb, None, row, comp_t),
                          (f"ocp_block_encode_t {name}", v + 1 + sb, f"composition encode_t {name}", row,
                           lambda tile=tile, sot=sot: ops.ocp_block_encode_t(x, fmt, tile, out=cot, scales_out=sot)),
                          (f"composition encode_both {name}", 4 * v + 2 + 2 * sb, None, row, comp_both),
                          (f"ocp_block_encode_both {name}", v + 2 + 2 * sb, f"composition encode_both {name}", row,
                           lambda tile=tile, so=so, sot=sot: ops.ocp_block_encode_both(x, fmt, tile, out=co, scales_out=so,
                                                                                       out_t=cot, scales_out_t=sot))]
            times = {c[0]: [] for c in cands}
            for _ in range(ROUNDS):
                for name, _, _, _, fn in cands:
                    times[name].append(_per_call(fn, reps))
            med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
            nbytes = {c[0]: c[1] for c in cands}
            spread = max(max(times[c[0]]) / min(times[c[0]]) for c in cands if c[3] is None)
            say(f"{list(shape)} {str(dtype).replace('torch.', '')}:")
            for name, b, replaces, yard, _ in cands:
                t = med[name]
                rounds = " ".join(f"{u * 1e6:8.1f}" for u in times[name])
                rate = b * n / t
                extra = ""
                if yard:
                    extra += f"   {t / med[yard]:5.3f} x {yard} (bytes {b / nbytes[yard]:5.3f})"
                if replaces:
                    ok = med[replaces] / t > spread
                    below, not_below = below + ok, not_below + (not ok)
                    extra += f"   {t / med[replaces]:5.3f} x the composition (bytes {b / nbytes[replaces]:5.3f})  " \
                             f"{'BELOW' if ok else 'NOT BELOW'}"
                say(f"  {name:34s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak"
                    f"{extra}")
            say(f"  round-to-round spread of the yardsticks (max / min): {spread:5.3f}")
            del x, co, cot, cands
            torch.cuda.empty_cache()
    say(f"new calls below the composition they replace by more than the yardsticks' spread: {below} BELOW, {not_below} NOT BELOW")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
