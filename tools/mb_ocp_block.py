#!/usr/bin/env python
"""Micro-benchmark of the tile-scaled hardware FP8 lane (csrc/fp8q_ocp_block.hip) next to its yardstick and to what it
replaces, on the same tensor and in the same process: [8192, 8192], float32 and bfloat16, E4M3FN, encode and quantize at each
tile.

  ocp_encode / ocp_quantize (per tensor, the range given)      the yardstick: the same bytes but for the scale table
  minmax + ocp_encode on x.view(-1, 128)                       1x128 today: two passes over x
  x.t().contiguous() + that pair                               128x1 today: three passes
  x.view(64, 128, 64, 128).permute(0, 2, 1, 3).contiguous() + that pair        128x128 today: three passes
  ocp_block_encode / ocp_block_quantize                        one pass, the range found inside it

Algorithmic bytes per element (v = 4 for float32, 2 for bfloat16): encode v + 1 (+ 4 / 128, 4 / 128, 4 / 16384 of scales),
the 1x128 composition 2v + 1, the two with a copy in front 4v + 1; quantize 2v, its compositions 3v and 5v.  (The compositions
of 128x1 and 128x128 leave codes in the copy's layout, not in x's: they are what a user can write today, not the same result.)

The candidates are interleaved: three rounds, each timing every candidate once as the time per call of `reps` back-to-back
calls between two HIP events (after a warm-up); medians are reported, and the largest round-to-round spread (max / min) of the
yardsticks.  No ratio is fixed in advance: each comparison says whether the new call lies below its composition by more than
that spread (BELOW) or does not (NOT BELOW), and the last line counts them.

    python tools/mb_ocp_block.py [--quick] [--out profiles/ocp_block_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

SHAPE = (8192, 8192)
ROUNDS = 3
PEAK = 8e12
TILES = ((1, 128), (128, 1), (128, 128))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocp_block_mb.txt"))
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = torch.float8_e4m3fn
    R, K = SHAPE
    n = R * K
    say(torch.cuda.get_device_name(0))
    say(f"tile-scaled OCP E4M3FN against the per-tensor lane and the compositions it replaces, {list(SHAPE)}; {ROUNDS} interleaved "
        f"rounds, time per call of {reps} back-to-back calls; TB/s over the algorithmic bytes, and as a fraction of "
        f"{PEAK / 1e12:.0f} TB/s")
    below = not_below = 0
    for dtype, v in ((torch.float32, 4), (torch.bfloat16, 2)):
        x = torch.randn(SHAPE, device="cuda").to(dtype)
        y = torch.empty_like(x)
        co = torch.empty(SHAPE, dtype=torch.uint8, device="cuda")
        mv1 = x.float().abs().amax().reshape(1)

        def view_of(tile):
            if tile == (1, 128):
                return lambda: x.view(-1, 128)
            if tile == (128, 1):
                return lambda: x.t().contiguous().view(-1, 128)
            return lambda: x.view(R // 128, 128, K // 128, 128).permute(0, 2, 1, 3).contiguous().view(-1, 128 * 128)

        def comp(tile, quant):
            rows = view_of(tile)

            def fn():
                t = rows()
                mv = ops.minmax(t, True, want_maxval=True)[2]
                if quant:
                    ops.ocp_quantize(t, mv, fmt, out=y)
                else:
                    ops.ocp_encode(t, mv, fmt, out=co, want_scale=True)
            return fn

        cands = [("ocp_encode per tensor", v + 1, None, None, lambda: ops.ocp_encode(x, mv1, fmt, out=co)),
                 ("ocp_quantize per tensor", 2 * v, None, None, lambda: ops.ocp_quantize(x, mv1, fmt, out=y))]
        for tile in TILES:
            name = f"{tile[0]}x{tile[1]}"
            so = torch.empty(ops._ocpb_geometry(SHAPE, tile)[2], dtype=torch.float32, device="cuda")
            sb = 4.0 * so.numel() / n
            passes = 1 if tile == (1, 128) else 3
            cands += [(f"composition encode {name}", (passes + 1) * v + 1 + sb, None, "ocp_encode per tensor", comp(tile, False)),
                      (f"ocp_block_encode {name}", v + 1 + sb, f"composition encode {name}", "ocp_encode per tensor",
                       lambda tile=tile, so=so: ops.ocp_block_encode(x, fmt, tile, out=co, scales_out=so)),
                      (f"composition quantize {name}", (passes + 2) * v, None, "ocp_quantize per tensor", comp(tile, True)),
                      (f"ocp_block_quantize {name}", 2 * v, f"composition quantize {name}", "ocp_quantize per tensor",
                       lambda tile=tile: ops.ocp_block_quantize(x, fmt, tile, out=y))]
        times = {c[0]: [] for c in cands}
        for _ in range(ROUNDS):
            for name, _, _, _, fn in cands:
                times[name].append(_per_call(fn, reps))
        med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
        nbytes = {c[0]: c[1] for c in cands}
        spread = max(max(times[c[0]]) / min(times[c[0]]) for c in cands if c[3] is None)
        say(f"{list(SHAPE)} {str(dtype).replace('torch.', '')}:")
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
            say(f"  {name:30s} rounds {rounds} us  median {t * 1e6:8.1f} us  {rate / 1e12:6.3f} TB/s  {rate / PEAK:5.3f} of peak{extra}")
        say(f"  round-to-round spread of the yardsticks (max / min): {spread:5.3f}")
        del x, y, co, cands
        torch.cuda.empty_cache()
    say(f"new calls below the composition they replace by more than the yardsticks' spread: {below} BELOW, {not_below} NOT BELOW")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
