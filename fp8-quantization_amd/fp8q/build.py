"""Compile csrc/*.hip -> csrc/libfp8q_hip.so for gfx950 (hipcc cross-compiles, no GPU needed).

Twenty-four translation units (the quantize / min-max family: long rows, short rows, k_rows_reg, the min/max reducers and the
multi-tensor plan; MSE grid, fused epilogue, storage codes, the float64 lane, the interval-histogram MSE search,
uniform INT quantization, the fp16 / bf16 lane, the FP quantizer's backward, the INT quantizers' backward, the INT quantizers' integer codes,
uniform INT quantization on fp16 / bf16, percentile selection, the storage codes of fp16 / bf16 tensors, the fused epilogue of the INT quantizers, the OCP E4M3FN / E5M2 lane, the block-scaled MX lane, the same lane with the blocks along dim 0, the OCP lane under a float32 scale per 1x128 / 128x1 / 128x128 tile, that lane's transposed operands) compiled in parallel and
linked into one library.  HEADERS are what they share; the code lanes' pieces are in fp8q_io.h (launch modes, element policies, the
FP8 conversion layer, the one I/O dispatcher), fp8q_half.h (the dword vectors, the half lane's helpers) and fp8q_intq.h (the INT
argument block, code packing); the two MX units share their device arithmetic through fp8q_mxq.h, the two OCP units theirs through fp8q_ocpq.h.  In-tree build: the .so is git-ignored but travels to the GPU box with the repo snapshot.
"""
import concurrent.futures
import os
import shutil
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "csrc")
SO = os.path.join(CSRC, "libfp8q_hip.so")
SOURCES = ["fp8q_quant.hip", "fp8q_rows.hip", "fp8q_rowsreg.hip", "fp8q_minmax.hip", "fp8q_multi.hip", "fp8q_mse.hip", "fp8q_epilogue.hip", "fp8q_codec.hip", "fp8q_f64.hip", "fp8q_mse_hist.hip",
           "fp8q_int.hip", "fp8q_h16.hip", "fp8q_grad.hip", "fp8q_intgrad.hip", "fp8q_intcodec.hip", "fp8q_inth16.hip", "fp8q_select.hip", "fp8q_codec_h16.hip", "fp8q_intepilogue.hip", "fp8q_ocp.hip", "fp8q_mx.hip", "fp8q_mx_t.hip", "fp8q_ocp_block.hip", "fp8q_ocp_block_t.hip"]
HEADERS = ["fp8q_common.h", "fp8q_percentile_ranks.h", "fp8q_rows.h", "fp8q_device.h", "fp8q_tables.h", "fp8q_bwd.h", "fp8q_intq.h", "fp8q_half.h", "fp8q_io.h", "fp8q_affine.h", "fp8q_mxq.h", "fp8q_ocpq.h", os.path.join("..", "..", "include", "fp8q.h")]
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, /opt/rocm/bin/hipcc, PATH)")


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    if not force and not needs_build():
        return SO
    hipcc = _hipcc()
    with tempfile.TemporaryDirectory(prefix="fp8q_build_") as tmp:
        def compile_one(src):
            obj = os.path.join(tmp, os.path.splitext(src)[0] + ".o")
            cmd = [hipcc] + CFLAGS + ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd, cwd=CSRC)
            return obj
        with concurrent.futures.ThreadPoolExecutor(max_workers=len(SOURCES)) as pool:
            objs = list(pool.map(compile_one, SOURCES))
        link = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", SO + ".tmp"]
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link, cwd=CSRC)
    os.replace(SO + ".tmp", SO)
    return SO


if __name__ == "__main__":
    print(build(force=True, verbose=True))
