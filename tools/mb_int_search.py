#!/usr/bin/env python
"""Micro-benchmark of the uniform quantizers' one-pass line search (fp8q_int_sse_grid_f32 / _f64, csrc/fp8q_int.hip) on
BASELINE config 1's size: 5 M Gauss samples, 1000 candidates, SymmetricUniformQuantizer(n_bits=8).

  step kernel   one process: ops.int_sse_grid on the float64 and the float32 sample, ops.mse_grid_f64 (E4M3, the existing
                FP search: the yardstick of the float64 lane) on the same float64 sample, and LineSearchEstimator's
                _candidate_losses (the call plus its one host read).  HIP events, median after a warm-up.
  step loop     a fresh child process with FP8Q_INT_KERNELS=0: the candidate loop this call replaces (deepcopy,
                set_quant_range, the eager torch chain, a reduction and a host read per candidate), same samples.
  step cqe      wall time of compute_quant_error.py (three distributions, five formats, 5 M samples), with the kernel
                and, in another child, with FP8Q_INT_KERNELS=0.

The driver starts every step as a child of its own under `timeout` and stops at the first one that fails.
Yardstick: the float64 call takes no longer than mse_grid_f64 on the same data (+10 % for box-to-box noise).

    python tools/mb_int_search.py [--quick] > profiles/int_search_mb.txt
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fp8-quantization_amd")
sys.path.insert(0, ROOT)
sys.path.insert(0, PKG)

N_CAND = 1000


def _events(fn, reps, warm=2):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    ts.sort()
    return ts[len(ts) // 2]


def _sample(n, dtype):
    """config 1's Gauss draw (ClippedGaussDistr, seed 10), float64 as the reference holds it"""
    import numpy as np
    import torch
    from quantization.distributions import ClippedGaussDistr
    np.random.seed(10)
    d = ClippedGaussDistr(params_dict={"mu": 0.0, "sigma": 1.0}, range_min=-10.0, range_max=10.0)
    return torch.as_tensor(d.sample((n,))).to(dtype).cuda()


def _estimator(x):
    from quantization.estimators import LineSearchEstimator
    from quantization.uniform import SymmetricUniformQuantizer
    est = LineSearchEstimator(quantizer=SymmetricUniformQuantizer(n_bits=8))
    est._define_search_range(x)
    return est


def step_kernel(n, reps):
    import numpy as np
    import torch
    from fp8q import ops
    print(torch.cuda.get_device_name(0))
    print(f"{n} Gauss samples, {N_CAND} candidates; median of {reps} by HIP events after 2 warm-up calls")
    x64 = _sample(n, torch.float64)
    est = _estimator(x64)
    thr = torch.from_numpy(np.float32(est.step_size * np.arange(1, N_CAND + 1))).view(-1, 1).cuda()
    out = torch.zeros(N_CAND, 1, dtype=torch.float64, device="cuda")
    t64 = _events(lambda: ops.int_sse_grid(x64, False, thr, 8, True, False, out=out), reps)
    fp = torch.zeros(1, N_CAND, 1, dtype=torch.float64, device="cuda")
    tfp = _events(lambda: ops.mse_grid_f64(x64, False, thr, [3.0], 8, 1, fp, reduce="sum"), reps)
    te64 = _events(lambda: est._candidate_losses(x64), reps)
    x32 = x64.float()
    est32 = _estimator(x32)
    t32 = _events(lambda: ops.int_sse_grid(x32, False, thr, 8, True, False, out=out), reps)
    te32 = _events(lambda: est32._candidate_losses(x32), reps)
    evals = float(n) * N_CAND
    print(f"  int_sse_grid float64 (INT8 symmetric)      {t64 * 1e3:9.3f} ms   {evals / t64 / 1e12:6.3f} T candidate-elements/s")
    print(f"  mse_grid_f64 (E4M3), same sample           {tfp * 1e3:9.3f} ms   {evals / tfp / 1e12:6.3f} T candidate-elements/s")
    print(f"  int_sse_grid float32                       {t32 * 1e3:9.3f} ms   {evals / t32 / 1e12:6.3f} T candidate-elements/s")
    print(f"  _candidate_losses float64 (call + read)    {te64 * 1e3:9.3f} ms")
    print(f"  _candidate_losses float32 (call + read)    {te32 * 1e3:9.3f} ms")
    ratio = t64 / tfp
    print(f"  float64 INT search / float64 FP search = {ratio:5.3f} (yardstick: <= 1.10) -> {'met' if ratio <= 1.10 else 'NOT met'}")
    return 0


def step_loop(n, reps):
    import torch
    assert os.environ.get("FP8Q_INT_KERNELS") == "0"
    print(f"the candidate loop (FP8Q_INT_KERNELS=0), {n} samples, {N_CAND} candidates; median of {reps} by HIP events after 1 warm-up call")
    for dtype in (torch.float64, torch.float32):
        x = _sample(n, dtype)
        est = _estimator(x)
        t = _events(lambda: est._candidate_losses(x), reps, warm=1)
        print(f"  _candidate_losses {str(dtype).replace('torch.', ''):8s} (loop)            {t * 1e3:9.1f} ms")
    return 0


def step_cqe(n):
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(PKG, "compute_quant_error.py"), "--n-samples", str(n)],
                       stdout=subprocess.DEVNULL)
    dt = time.perf_counter() - t0
    route = "candidate loop (FP8Q_INT_KERNELS=0)" if os.environ.get("FP8Q_INT_KERNELS") == "0" else "one-pass INT search"
    print(f"  compute_quant_error.py --n-samples {n}, {route}: wall {dt:7.1f} s (exit {p.returncode})")
    return p.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="500 k samples, fewer repetitions")
    ap.add_argument("--step", choices=["kernel", "loop", "cqe"])
    a = ap.parse_args()
    n = 500_000 if a.quick else 5_000_000
    if a.step == "kernel":
        return step_kernel(n, 3 if a.quick else 7)
    if a.step == "loop":
        return step_loop(n, 1 if a.quick else 3)
    if a.step == "cqe":
        return step_cqe(n)
    me = [sys.executable, os.path.abspath(__file__)] + (["--quick"] if a.quick else [])
    eager = dict(os.environ, FP8Q_INT_KERNELS="0")
    steps = [("kernel", 240, os.environ), ("loop", 300, eager), ("cqe", 420, os.environ), ("cqe", 420, eager)]
    for name, limit, env in steps:
        sys.stdout.flush()
        rc = subprocess.run(["timeout", "-k", "10", str(limit)] + me + ["--step", name], env=dict(env)).returncode
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping here")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
