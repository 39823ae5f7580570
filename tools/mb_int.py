#!/usr/bin/env python
"""Micro-benchmark of the uniform (INT) quantizers on the HIP kernels (csrc/fp8q_int.hip) next to the eager torch chain
(FP8Q_INT_KERNELS=0) on the same tensors:

  * INT8 quantize with fixed ranges, per tensor and per channel, on [2^21,3,7,7] and [64,64,112,112] fp32: time per call by
    events (median of 20) and the fraction of 8 TB/s over the 8 B per element the kernel moves;
  * an INT8 ResNet-18 and MobileNetV2 (symmetric per-channel weights with current_minmax, running_minmax activations,
    batch 8 x 3 x 64 x 64): calibration pass and validation forward, wall time per call.

    python tools/mb_int.py [--quick]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "fp8-quantization_amd"))

import torch  # noqa: E402

HBM = 8.0e12


def _events(fn, reps):
    for _ in range(3):
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


def _env(on):
    if on:
        os.environ.pop("FP8Q_INT_KERNELS", None)
    else:
        os.environ["FP8Q_INT_KERNELS"] = "0"


def kernels(reps):
    from quantization.uniform import SymmetricUniformQuantizer, AsymmetricUniformQuantizer
    for shape in ((1 << 21, 3, 7, 7), (64, 64, 112, 112)):
        x = torch.randn(shape, device="cuda")
        for pc in (False, True):
            for cls in (SymmetricUniformQuantizer, AsymmetricUniformQuantizer):
                q = cls(n_bits=8, per_channel=pc)
                if pc:
                    mn, mx = x.view(shape[0], -1).aminmax(dim=1)
                else:
                    mn, mx = x.aminmax()
                q.set_quant_range(mn, mx)
                with torch.no_grad():
                    _env(True)
                    tk = _events(lambda: q(x), reps)
                    _env(False)
                    te = _events(lambda: q(x), reps)
                    _env(True)
                frac = 8.0 * x.numel() / tk / HBM
                print(f"{cls.__name__[:4]:4s} {'per-channel' if pc else 'per-tensor ':11s} {str(list(shape)):20s} "
                      f"kernel {tk * 1e6:9.1f} us  {frac:5.3f} of 8 TB/s   eager chain {te * 1e6:9.1f} us  ({te / tk:4.1f}x)")
        del x
        torch.cuda.empty_cache()


def models(reps):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from quantization.quantization_manager import QMethods
    from quantization.range_estimators import RangeEstimators
    for arch in ("resnet18", "mobilenet_v2"):
        for on in (True, False):
            _env(on)
            torch.manual_seed(0)
            kw = dict(method=QMethods.symmetric_uniform.cls, act_method=QMethods.symmetric_uniform.cls,
                      weight_range_method=RangeEstimators.current_minmax.cls,
                      act_range_method=RangeEstimators.running_minmax.cls, n_bits=8, n_bits_act=8,
                      per_channel_weights=True)
            if arch == "resnet18":
                from models.resnet import resnet18
                from models.resnet_quantized import QuantizedResNet
                net = QuantizedResNet(resnet18(), input_size=(1, 3, 64, 64), **kw)
            else:
                from models.mobilenet_v2 import MobileNetV2
                from models.mobilenet_v2_quantized import QuantizedMobileNetV2
                net = QuantizedMobileNetV2(MobileNetV2(input_size=64), input_size=(1, 3, 64, 64), **kw)
            net = net.cuda().eval()
            net.quantized_weights()
            net.quantized_acts()
            x = torch.randn(8, 3, 64, 64, device="cuda")
            with torch.no_grad():
                net.estimate_ranges()

                def calib():
                    net(x)
                torch.cuda.synchronize()
                tc = _wall(calib, reps)
                net.fix_ranges()
                tv = _wall(calib, reps)
            print(f"{arch:12s} {'kernels' if on else 'eager  '}  calibration pass {tc * 1e3:7.3f} ms   "
                  f"validation forward {tv * 1e3:7.3f} ms")
    _env(True)


def _wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    reps = 5 if a.quick else 20
    print(torch.cuda.get_device_name(0))
    kernels(reps)
    models(reps)


if __name__ == "__main__":
    main()
