"""Two builds of the library in ONE process (same device state for both), alternating blocks of calls, HIP-event timed: fused
min/max + quantize on [2^k,147] (k_rows_staged) and the 1 GiB copy (k_copy, the control):

    python tools/ab_fused_copy.py OLD.so NEW.so [k = 21]"""
import ctypes, os, statistics, sys
import torch
if len(sys.argv) < 3:
    sys.exit(__doc__)
libs = {"parent": ctypes.CDLL(os.path.abspath(sys.argv[1])), "child": ctypes.CDLL(os.path.abspath(sys.argv[2]))}
vp, i64, f32, ci = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_int
for L in libs.values():
    L.fp8q_minmax_quantize_f32.argtypes = [vp, vp, i64, i64, vp, vp, vp, f32, ci, ci, vp]
    L.fp8q_minmax_quantize_f32.restype = ci
    L.fp8q_copy_f32.argtypes = [vp, vp, i64, vp]
    L.fp8q_copy_f32.restype = ci
dev = torch.device("cuda")
C, inner = 1 << (int(sys.argv[3]) if len(sys.argv) > 3 else 21), 147
x = torch.randn(C * inner, device=dev)
y = torch.empty_like(x)
r = torch.empty(3, C, device=dev)
n_copy = 1 << 28
xc = x[:n_copy] if x.numel() >= n_copy else torch.randn(n_copy, device=dev)
yc = y[:n_copy] if y.numel() >= n_copy else torch.empty(n_copy, device=dev)
st = torch.cuda.current_stream().cuda_stream
def fused(L):
    rc = L.fp8q_minmax_quantize_f32(x.data_ptr(), y.data_ptr(), C, inner, r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), 2.0, 8, 1, st)
    assert rc == 0, rc
def copy(L):
    rc = L.fp8q_copy_f32(xc.data_ptr(), yc.data_ptr(), n_copy, st)
    assert rc == 0, rc
CALLS, BLOCKS = 20, 40
for name, fn in (("fused_minmax_quant [%d,147] E5M2" % C, fused), ("copy 1 GiB", copy)):
    for L in libs.values():
        for _ in range(10):
            fn(L)
    torch.cuda.synchronize()
    res = {"parent": [], "child": []}
    for b in range(BLOCKS):
        order = ("parent", "child") if b % 2 == 0 else ("child", "parent")
        for tag in order:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(CALLS + 1)]
            ev[0].record()
            for k in range(CALLS):
                fn(libs[tag])
                ev[k + 1].record()
            torch.cuda.synchronize()
            res[tag].append(statistics.median(ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(CALLS)))
    print(name + ": %d alternating blocks of %d calls per library, median us of each block" % (BLOCKS, CALLS))
    for tag in ("parent", "child"):
        v = sorted(res[tag])
        print("  %-6s min %.1f  p25 %.1f  median %.1f  p75 %.1f  max %.1f" % (tag, v[0], v[len(v) // 4], statistics.median(v), v[3 * len(v) // 4], v[-1]))
    d = [c - p for p, c in zip(res["parent"], res["child"])]
    print("  child - parent per block pair: median %+.2f us, min %+.2f, max %+.2f" % (statistics.median(d), min(d), max(d)))
    sys.stdout.flush()
