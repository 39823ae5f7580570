#!/usr/bin/env python3
"""One call per launch site of the fp32 quantize / min-max family (fp8q_quant / rows / rowsreg / minmax / multi .hip), each at
the smallest shape that takes that site: which kernel the host picks, with what grid, workgroup and LDS.

    timeout -k 10 200 rocprofv3 --kernel-trace --output-format csv -d OUT -o routes -- python tools/route_shapes.py run
    python tools/route_shapes.py reduce OUT > routes.txt      # (kernel, grid, workgroup, LDS) in launch order + families

FP8Q_SO selects the library, so two builds can be traced and their reduced files compared with diff.
"""
import csv
import glob
import os
import re
import sys

FAMILIES = ["k_quant_rows", "k_quant_scalar", "k_quant_rows_dm", "k_quant_scalar_dm", "k_quant_short_rows_dm", "k_quant_rows_sel",
            "k_copy", "k_rows_direct", "k_rows_flat", "k_rows_staged", "k_rows_staged_mm", "k_rows_reg", "k_small_rows_fused",
            "k_minmax_partial", "k_ranges_unpack", "k_sign_fold", "k_multi_flat", "k_multi_rowmax"]


def run():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fp8-quantization_amd"))
    import torch
    from fp8q import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(0)

    def rnd(*shape, off=0):
        """[shape] float32; off = 1: the data starts one float past a 16-byte boundary"""
        n = 1
        for s in shape:
            n *= s
        return torch.randn(n + off, device=dev, generator=g)[off:].view(*shape)

    def buf(*shape, off=0):
        n = 1
        for s in shape:
            n *= s
        return torch.empty(n + off, device=dev)[off:].view(*shape)

    one = torch.tensor([2.5], device=dev)

    def mv(C):
        return torch.rand(C, device=dev, generator=g) + 1.0

    # per-tensor K1
    ops.quantize(rnd(4101), one, 3)
    ops.quantize(rnd(4101), one, 3, out=buf(4101, off=1))                 # k_quant_scalar
    ops.quantize(rnd((8 << 20) + 4), one, 3)                               # U = kUnroll
    ops.quantize(rnd((16 << 20) + 4), one, 3)                              # nontemporal (>= 64 MiB)
    # per-channel K1
    ops.quantize(rnd(4096, 147), mv(4096), 3)                              # flat
    ops.quantize(rnd(4096, 147, off=1), mv(4096), 3, out=buf(4096, 147, off=1))   # direct
    ops.quantize(rnd(64, 3), mv(64), 3)                                    # direct, no table
    ops.quantize(rnd(8, 4608), mv(8), 3)                                   # 2-D k_quant_rows
    ops.quantize(rnd(8, 4608), mv(8), 3, out=buf(8, 4608, off=1))          # 2-D k_quant_scalar
    # dm / ds / dms
    mb = torch.tensor([3.0], device=dev)
    flag = torch.ones(1, dtype=torch.uint8, device=dev)
    for sel in ((mb, 1), (3, flag), (mb, flag)):
        ops.quantize(rnd(4101), one, sel[0], sign_bits=sel[1])
        ops.quantize(rnd(4101), one, sel[0], sign_bits=sel[1], out=buf(4101, off=1))
        ops.quantize(rnd(96, 9), mv(96), sel[0], sign_bits=sel[1])         # wave per row
        ops.quantize(rnd(8, 4608), mv(8), sel[0], sign_bits=sel[1])
    # select: the last launch of an MSE calibration step with a mantissa search
    cal = ops.MseCalibration(1, dev, [2, 3, 4], 8, 1, n_cand=16)
    cal.step(rnd(1, 65536))
    # min/max
    ops.minmax(rnd(512, 576), True)                                        # reg
    ops.minmax(rnd(4096, 147), True)                                       # staged_mm
    ops.minmax(rnd(64, 3), True)                                           # direct
    ops.minmax(rnd(2 << 20), False)                                        # split rows + reducer block
    ops.minmax(rnd(4096, 147), True, packed=ops.new_packed(4096, dev))
    ops.minmax_linspace(rnd(2 << 20), False, steps=16)
    pk = ops.new_packed(64, dev)
    ops.minmax(rnd(64, 3), True, packed=pk)
    ops.ranges_unpack(pk)
    ops.sign_fold(rnd(64))
    # min/max + quantize
    for inner in (9, 100, 147, 200, 400):                                  # k_small_rows_fused, every EPL
        ops.minmax_quantize(rnd(16, inner), 3)
    for shape in ((512, 576), (256, 1152), (64, 4608)):                    # reg
        ops.minmax_quantize(rnd(*shape), 3)
    ops.minmax_quantize(rnd(65536, 147), 3)                                # staged
    ops.minmax_quantize(rnd(4096, 256), 3)                                 # reg again: 16 lanes x 4 slots are 100 % filled
    ops.minmax_quantize(rnd(4096, 32), 3)                                  # k_rows_flat<1>: too short for reg, 130 table rows
                                                                           # per chunk outgrow k_rows_staged's LDS budget
    x = rnd(4096, 147)
    ops.minmax_quantize(x, 3, out=x)                                       # in place
    ops.minmax_quantize(rnd(512, 577), 3)                                  # direct fused
    # codec
    codes = ops.encode(rnd(4096, 147), mv(4096), 3)
    ops.decode(codes, mv(4096), 3)
    # multi-tensor plan: five tensors, one misaligned, modes 0 / 3 / 4, and the range + quantize pair
    shapes = [(64, 147), (128, 576), (256, 1152), (32, 27), (100, 100)]
    items = [(rnd(*s, off=1 if i == 2 else 0), mv(s[0]), 3) for i, s in enumerate(shapes)]
    ops.multi_quantize(items)
    enc = ops.multi_minmax_encode([(it[0], torch.empty(it[0].shape[0], device=dev), 3) for it in items])
    ops.multi_decode([(c, mv(c.shape[0]), 3, 8, 1, buf(*c.shape, off=1 if i == 2 else 0)) for i, c in enumerate(enc)])
    ops.multi_minmax_quantize([(it[0], torch.empty(it[0].shape[0], device=dev), 3) for it in items])
    ops.MultiPlan([(rnd(*s), mv(s[0]), 3) for s in shapes]).launch()
    ops.copy(rnd(4096 * 5))
    torch.cuda.synchronize()
    print("route_shapes: done")


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", name)


def reduce(outdir):
    rows = []
    for path in glob.glob(os.path.join(outdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lds = next((k for k in (rows[0] if rows else {}) if "LDS" in k.upper()), None)
    seen = set()
    for r in rows:
        name = short(r["Kernel_Name"])
        if not re.match(r"k_[a-z0-9_]+(<.*>)?$", name):
            continue        # torch's own kernels (random inputs, fills)
        seen.add(name.split("<")[0])
        print("%-52s grid %s x %s x %s  wg %s  lds %s" % (name, r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"],
                                                         r["Workgroup_Size_X"], r[lds] if lds else "?"))
    print("families seen: %d of %d" % (len(seen & set(FAMILIES)), len(FAMILIES)))
    for fam in FAMILIES:
        if fam not in seen:
            print("  NOT SEEN: " + fam)


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "reduce":
        reduce(sys.argv[2])
    else:
        sys.exit(__doc__)
