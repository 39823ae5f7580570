"""bench.py as the driver runs it: the JSON-line contract, the bare multi-rank self-launch, configs 3 / 4 in `extras`."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, timeout):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):      # a bare invocation: no launcher environment
        env.pop(k, None)
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)


def _line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, stdout[-3000:]
    return json.loads(lines[0])


def test_bare_multi_gpu_invocation_starts_its_ranks_cpu():
    """`python bench.py --gpus 2` with no launcher must start 2 ranks itself (it used to sys.exit with a hint).  Without a
    GPU a rank then refuses -- the engine has no CPU path -- and the launcher's failure report (ChildFailedError naming
    bench.py) shows that the ranks were started by torch.distributed.run; exit code non-zero.  (The launcher stops the
    other rank as soon as the first one has failed, so the second refusal is not always printed.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-side check of the launcher; the GPU box runs the real thing below")
    r = _run(["--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "0"], 600)
    assert r.returncode != 0
    out = r.stdout + r.stderr
    assert out.count("bench.py needs a GPU") >= 1, out[-3000:]
    assert "ChildFailedError" in out and "bench.py FAILED" in out, out[-3000:]
    assert "launch with: python -m torch.distributed.run" not in r.stdout + r.stderr


def test_dry_run_eight_ranks_cpu():
    """the world size the driver's scaling run ends with: 8 gloo ranks walk the same call sequence; a rank ships 1/8 of the
    model as 1-byte codes in ONE all-gather and the calibration flow still has exactly one 16-byte all-reduce"""
    r = _run(["--dry-run-ranks", "8"], 900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"dry_run"' in ln][0])
    assert d["ranks"] == 8 and d["ranks_seen"] == 8
    seq = d["call_sequence_as_executed"]
    head = seq["headline: quantize_weight_sharded_codes(fixed ranges)"]
    assert len(head) == 1 and head[0]["dtype"] == "uint8" and head[0]["send_bytes"] == 1024 * 147
    full = d["full_size_bytes"]["headline (value at --gpus N)"]["all_gather_into_tensor codes"]
    assert full["received_per_rank"] == 7 * (1 << 21) * 147 <= 7 / 8 * 8 * (1 << 21) * 147
    r18 = seq["resnet18_weights_one_allgather: quantize_weights_sharded_bucketed (REAL shapes)"]
    assert len(r18) == 1 and r18[0]["dtype"] == "uint8" and abs(r18[0]["send_bytes"] - (11678912 + 4800 * 4) / 8) < 0.01 * 11678912 / 8
    assert seq["c5: calibrate_quantize_sharded"] == [dict(op="all_reduce", dtype="float32", send_bytes=16, reduce="MAX")]


def test_dry_run_ranks_prints_the_call_sequence_cpu():
    """`python bench.py --dry-run-ranks 4`: no GPU, 4 gloo ranks, the N-rank call sequence of the bench (headline flow,
    codes variant, ResNet-18 bucketed all-gather at its real shapes, config 5) with every collective's byte count."""
    r = _run(["--dry-run-ranks", "4"], 900)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{") and '"dry_run"' in ln]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["ranks"] == 4 and d["ranks_seen"] == 4
    seq = d["call_sequence_as_executed"]
    # the headline ships 1-byte codes of fixed-range channels: ONE collective, a quarter of the fp32 form's bytes, no ranges
    head = seq["headline: quantize_weight_sharded_codes(fixed ranges)"]
    assert [c["op"] for c in head] == ["all_gather_into_tensor"] and head[0]["dtype"] == "uint8"
    assert head[0]["send_bytes"] == 1024 * 147
    head32 = seq["headline, fp32 wire (value_fp32_wire): quantize_weight_sharded(fixed ranges)"]
    assert [c["op"] for c in head32] == ["all_gather_into_tensor", "all_gather_into_tensor"]
    assert head32[0]["send_bytes"] == 1024 * 147 * 4 and head32[1]["send_bytes"] == 1024 * 4
    codes = seq["weights_allgather.codes_u8: quantize_weight_sharded_codes"]
    assert codes[0]["dtype"] == "uint8" and codes[0]["send_bytes"] == 1024 * 147
    r18 = seq["resnet18_weights_one_allgather: quantize_weights_sharded_bucketed (REAL shapes)"]
    # 1/4 of the model per rank, as 1-byte codes + fp32 ranges (round 5: the default wire form); the fp32 form is 4 x that
    assert len(r18) == 1 and r18[0]["dtype"] == "uint8" and abs(r18[0]["send_bytes"] - (11678912 + 4800 * 4) / 4) < 0.01 * 11678912 / 4
    r18f = seq["resnet18_weights_one_allgather, fp32 wire (round 4's form)"]
    assert len(r18f) == 1 and r18f[0]["dtype"] == "float32" and abs(r18f[0]["send_bytes"] - (11678912 + 4800) * 4 / 4) < 0.01 * 11678912
    c5 = seq["c5: calibrate_quantize_sharded"]
    assert c5 == [dict(op="all_reduce", dtype="float32", send_bytes=16, reduce="MAX")]
    full = d["full_size_bytes"]["headline (value at --gpus N)"]
    assert full["all_gather_into_tensor codes"]["send_bytes_per_rank"] == (1 << 21) * 147
    assert full["all_gather_into_tensor codes"]["received_per_rank"] == 3 * (1 << 21) * 147 <= 3 / 4 * 4 * (1 << 21) * 147
    full32 = d["full_size_bytes"]["headline, fp32 wire (value_fp32_wire)"]
    assert full32["all_gather_into_tensor values"]["received_per_rank"] == 3 * (1 << 21) * 147 * 4


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stdout + r.stderr


@pytest.mark.gpu
def test_bare_two_rank_gloo_bench_on_one_gpu():
    """The multi-process path end to end on the one-GPU box: bare `python bench.py --gpus 2 --backend gloo` re-executes
    itself through torch.distributed.run, both ranks share cuda:0, every section of the line is produced and the
    collectives saw 2 ranks.  (gloo carries device tensors through the host: its times say nothing about xGMI.)"""
    r = _run(["--gpus", "2", "--backend", "gloo", "--steps", "3", "--warmup", "1", "--channels-per-gpu", "65536", "--full"], 1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    line = _line(r.stdout)
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["scaling"] == "weak"
    # `value` is north_star's weight flow END TO END (shard -> quantize -> all-gather): it contains the collective
    for k in ("value_kernel_only", "kernel_us", "collective_us", "xgmi_bytes_received_per_rank", "xgmi_gb_s",
              "value_codes_wire", "value_resnet18_strong", "value_c5", "value_fp32_wire", "fp32_wire_ms_per_step", "wire"):
        assert k in line, k
    assert line["collective_us"] > 0 and line["kernel_us"] > 0
    assert line["ms_per_step"] * 1e3 >= line["kernel_us"] + 0.9 * line["collective_us"]      # the step time holds both phases
    assert line["value"] < line["value_kernel_only"]
    n_total = 2 * 65536 * 147
    assert abs(line["value"] - n_total / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.02 * line["value"]
    assert line["xgmi_bytes_received_per_rank"] == 65536 * 147 and line["xgmi_gb_s"] is None   # 1-byte codes; gloo: no xGMI figure
    assert line["fp32_wire_xgmi_bytes_received_per_rank"] == (65536 * 147 + 65536) * 4 and line["value_fp32_wire"] > 0
    assert "REDUCED" in line["config"]["workload"] and "INCLUDES the collective" in line["config"]["parallelism"]
    nsp = line["north_star_path"]
    assert nsp["ranks_seen"] == 2
    assert nsp["weights_allgather"]["fp32"]["collective_us"] > 0
    assert nsp["c5"]["collective_us"] > 0 and nsp["c5"]["gelem_s"] > 0
    assert nsp["resnet18_weights_one_allgather"]["tensors"] == 21
    assert "cpu_baseline" not in line and "extras" not in line          # rank 0 at N = 1 only


@pytest.mark.gpu
def test_single_gpu_line_carries_roofline_cpu_baseline_and_model_configs():
    """N = 1 as the driver runs it (fewer steps): the contract's keys, `roofline`, `cpu_baseline` (the C port + the
    reference-equivalent eager chain), and BASELINE configs 3 / 4 under `extras`."""
    r = _run(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--no-north-star-path"], 1500)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    line = _line(r.stdout)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 20 and line["ranks_seen"] == 1
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3 and rf["frac"] > 0.5
    # HBM traffic from the PMC counters, measured by the run itself (two rocprofv3 --pmc passes): no wasted re-reads
    # (if the profiler cannot run nested on some box, the line falls back to the recorded figure and says so)
    assert rf["traffic_source"].startswith("measured in this run") or "profiles/pmc_traffic.json" in rf["traffic_source"], \
        rf["traffic_source"]
    assert 0.98 < rf["traffic"] / rf["algorithmic_bytes_per_launch"] < 1.05
    cb = line["cpu_baseline"]
    # value = the reference's CPU path (eager ATen chain), where the driver's parser keeps it; the fused C port next to it
    assert cb["kind"] == "reference-equivalent" and cb["value"] > 0 and cb["cores"] >= 1 and cb["unit"] == "Gelem/s"
    assert cb["port_kind"] == "port" and cb["port_value"] > cb["value"] and cb["gpu_output_bit_exact_on_sample"] is True
    ex = line["extras"]
    c3, c4 = ex["c3_resnet18_b64"], ex["c4_mobilenetv2_b64"]
    v3 = c3["validation_forward"]
    # the reference's launch pattern: 21 weight + 30 activation quantizer calls, 218.9 M elements
    assert v3["reference_pattern"]["launches"] == 51
    assert abs(v3["reference_pattern"]["elements"] - 218.9e6) / 218.9e6 < 0.01
    assert abs(v3["reference_pattern"]["algorithmic_gb"] - 1.751) < 0.02
    assert v3["default"]["launches"] < v3["cache0_fused"]["launches"] <= 51
    assert c3["calibration_batch"]["launches"] >= 51
    v4 = c4["validation_forward"]
    assert v4["reference_pattern"]["launches"] == 117
    assert abs(v4["reference_pattern"]["elements"] - 444.9e6) / 444.9e6 < 0.01
    for key, n_m in (("calibration_batch_fixed_mantissa", 1), ("calibration_batch_mantissa_search_6", 6)):
        cal = c4[key]
        by = cal["by_entry"]
        # one library call per MSE quantizer: search + selection + quantization, behind a BN with the epilogue in the same call
        n_calls = by.get("mse_calibrate", {}).get("calls", 0) + by.get("mse_calibrate_fused_epilogue", {}).get("calls", 0)
        assert n_calls in (116, 117) and by["mse_calibrate_fused_epilogue"]["calls"] >= 50 and cal["k4_t_cand_elem_s"] > 0, key
        assert cal["wall_ms"] > 0 and cal["host_enqueue_ms"] <= cal["wall_ms"] and cal["fix_ranges_ms"] > 0
    assert c4["calibration_batch_mantissa_search_6"]["library_us"] > c4["calibration_batch_fixed_mantissa"]["library_us"]
    # the metric's second half ("ResNet-18 PTQ top-1 delta") as this box can show it: the oracle recomputes every quantizer
    # launch of a validation batch inside the GPU model -> identical logits -> zero delta attributable to the kernels
    for c in (c3, c4):
        assert c["logits_bit_identical_with_oracle_quantizers"] is True and c["quantized_weights_bit_identical_with_oracle"] is True
        assert c["top1_delta_attributable_to_kernels"] == 0
        assert 0.0 <= c["argmax_agreement_with_fp32"] <= 1.0 and c["weights_checked"] >= 21


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and reports the headline alone; --dump-outputs writes the
    last step's output: a seeded float32 sample of whole channels and float64 sums over channel groups, under 64 MB."""
    import numpy as np
    r = _run(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)], 600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    line = _line(r.stdout)
    assert line["steps"] == 7 and line["ms_per_step"] > 0 and line["unit"] == "Gelem/s" and line["dtype"] == "f32"
    assert abs(line["value"] - (1 << 21) * 147 / (line["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * line["value"]
    for k in ("cpu_baseline", "extras", "north_star_path"):
        assert k not in line, k
    assert "NOT measured in this run" in line["roofline"]["traffic_source"]
    files = sorted(os.listdir(tmp_path))
    assert files == ["y_group_sums.npy", "y_sample.npy"], files
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 << 20
    ys, sums = np.load(tmp_path / "y_sample.npy"), np.load(tmp_path / "y_group_sums.npy")
    assert ys.dtype == np.float32 and ys.shape == (1 << 16, 3, 7, 7) and np.isfinite(ys).all() and ys.any()
    assert sums.dtype == np.float64 and sums.shape == (1 << 20,) and np.isfinite(sums).all()
