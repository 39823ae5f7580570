#!/usr/bin/env python
"""Micro-benchmark of ops.mx_grouped_matmul (csrc/fp8q_mx_mm_grouped.hip): G = 32 experts of W [4096, 4096], T = 64 ... 8192
rows in uniform groups; E4M3FN x E4M3FN, E4M3FN x E2M1 and E2M1 x E2M1 (activations x weights).  Per shape and pair, timed
next to each other:
  (a) one mx_grouped_matmul, float32 out, workspace passed by the caller: by the plan, and with tile_m forced to 32 and 128;
  (b) G calls of mx_matmul on slices, the group sizes already on the host (the sync that this route needs is NOT timed);
  (c) the same loop with skinny=True where a group has at most 64 rows (omitted otherwise: it would be (b));
  (d) G torch.matmul calls on slices of operands already decoded to bfloat16 -- the yardstick, whose round-to-round spread is
      printed.
Every candidate rotates through distinct sets of the G weight matrices whose total exceeds 512 MiB, so that every call reads
its W from HBM and not from the 256 MiB last-level cache.  The candidates are interleaved: ROUNDS rounds, each timing every
candidate once as the time per call over a window of about 100 ms of back-to-back calls between two HIP events (after a
warm-up); medians.  A ratio
within the printed spread of 1 is no difference.  (a) is also given as bytes of W (codes + scales of all G experts) over the
CALL time -- both launches and their gap included; it is not kernel time -- and as a share of 8 TB/s.  Needs a GPU.

    python tools/mb_mx_grouped.py [--quick] [--t 64 512 8192] [--out profiles/mx_grouped_mb.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

ROUNDS, G, N, K, HBM = 5, 32, 4096, 4096, 8.0e12
E4M3, E2M1 = torch.float8_e4m3fn, torch.float4_e2m1fn_x2
PAIRS = [("e4m3fn x e4m3fn", E4M3, E4M3), ("e4m3fn x e2m1", E4M3, E2M1), ("e2m1 x e2m1", E2M1, E2M1)]


def _per_call(fn, n_w, reps):
    """fn(i) uses weight set i % n_w; warm-up and the timed calls walk the ring"""
    for i in range(min(reps, 2)):
        fn(i % n_w)
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
    ap.add_argument("--t", type=int, nargs="*", default=[64, 512, 1024, 2048, 8192])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mx_grouped_mb.txt"))
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(torch.cuda.get_device_name(0))
    say(f"y[o_g : o_g+1] = X[o_g : o_g+1, {K}] . W[g, {N}, {K}]^T, G = {G} uniform groups; {ROUNDS} interleaved rounds, W rotating "
        f"over > 512 MiB per candidate, medians of the time per call in us.  (a) mx_grouped_matmul by the plan, (a32) / (a128) "
        f"tile_m forced  (b) G x mx_matmul on slices  (c) the same, skinny=True  (d) G x torch.matmul on decoded bfloat16")
    w = torch.randn((G * N, K), device="cuda")
    wd = ops.mx_decode(*ops.mx_encode(w, E4M3), out_dtype=torch.bfloat16).view(G, N, K)     # 1 GiB: one set is a ring
    for name, fx, fw in PAIRS:
        wbytes = G * N * K * (1 if fw == E4M3 else 0.5) + G * N * K // 32
        n_w = int(512 * 2 ** 20 // wbytes) + 2      # two sets at least: one E4M3 set alone is 528 MiB
        sets = [tuple(t.view(G, N, -1) for t in ops.mx_encode(w, fw)) for _ in range(n_w)]
        for T in a.t:
            c = T // G
            xc, xs = ops.mx_encode(torch.randn((T, K), device="cuda"), fx)
            xd = ops.mx_decode(xc, xs, out_dtype=torch.bfloat16)
            off = torch.arange(0, T + 1, c, dtype=torch.int32, device="cuda")
            y = torch.empty((T, N), device="cuda")
            xg = [(xc[g * c:(g + 1) * c], xs[g * c:(g + 1) * c], xd[g * c:(g + 1) * c], y[g * c:(g + 1) * c]) for g in range(G)]
            cands = []
            for tm in (None, 32, 128):
                plan = ops.mx_grouped_plan(T, N, K, G, tm)
                wk = torch.empty(plan[2], dtype=torch.uint8, device="cuda")
                cands.append((f"a{tm or ''}", n_w, lambda i, tm=tm, wk=wk: ops.mx_grouped_matmul(
                    xc, xs, *sets[i], off, out=y, tile_m=tm, workspace=wk)))

            def loop(i, **kw):
                for g in range(G):
                    ops.mx_matmul(xg[g][0], xg[g][1], sets[i][0][g], sets[i][1][g], out=xg[g][3], **kw)

            cands.append(("b", n_w, loop))
            if c <= ops.MX_SKINNY_MAX_M:
                sk = torch.empty(max(ops.mx_skinny_plan(c, N, K)[3], 16), dtype=torch.uint8, device="cuda")
                cands.append(("c", n_w, lambda i: loop(i, skinny=True, workspace=sk)))
            cands.append(("d", 1, lambda i: [torch.matmul(xg[g][2], wd[g].t()) for g in range(G)]))
            times = {k[0]: [] for k in cands}
            window = 0.02 if a.quick else 0.1
            reps = {kind: max(2 * ring, int(window / _per_call(fn, ring, 2 * ring))) for kind, ring, fn in cands}
            for _ in range(ROUNDS):
                for kind, ring, fn in cands:
                    times[kind].append(_per_call(fn, ring, reps[kind]))
            med = {k: sorted(t)[len(t) // 2] for k, t in times.items()}
            spread = max(times["d"]) / min(times["d"])
            say(f"[T {T:4d} = {G} x {c:3d}] {name:16s} " + "  ".join(f"({k}) {v * 1e6:7.1f}" for k, v in med.items())
                + f"   (a)/(b) {med['a'] / med['b']:5.3f}  (a32)/(a128) {med['a32'] / med['a128']:5.3f}  spread of (d) {spread:5.3f}  "
                f"(b) max/min {max(times['b']) / min(times['b']):5.3f}   (a): plan (tile_m, m_tiles_max) "
                f"{ops.mx_grouped_plan(T, N, K, G)[:2]}, W {wbytes / 2 ** 20:5.0f} MiB per call, "
                f"{wbytes / med['a'] * 1e-12:5.2f} TB/s of call time, {100.0 * wbytes / med['a'] / HBM:4.1f} % of 8 TB/s")
        del sets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
