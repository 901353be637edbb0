"""The bench line the driver parses: the committed `profiles/r06_bench_n1.json` (an unedited `python bench.py --full` line; its
`roofline.traffic` is what bench.py itself reads from profiles/r06_traffic.json) must carry every field of the measurement contract,
and the roofline numbers must be self-consistent and agree with the committed rocprofv3 summaries of the same build."""
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_committed_bench_line_follows_the_contract():
    d = json.loads((ROOT / "profiles" / "r06_bench_n1.json").read_text())
    base = json.loads((ROOT / "BASELINE.json").read_text())
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic"
    assert d["vs_baseline"] is None                      # BASELINE.md holds no published number for this metric
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["dtype"] == "fp16"                          # the dtype that holds 1e-3 on the full-depth planted golden (tests/test_fp16_gpu.py)
    if isinstance(base.get("metric"), str):
        assert d["unit"].split("/")[0] in base["metric"] or "images" in d["unit"]
    # value is whole-job throughput: batch / step time
    assert abs(d["value"] - d["config"]["batch"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["alg_flops_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12) / r["achieved"] < 2e-2
    assert r["traffic"] is None or r["traffic"] > 0.5 * r["alg_bytes_per_launch"]
    # frac prices ALGORITHMIC flops: the class's launches x alg_flops_per_launch cannot exceed the whole step's
    # algorithmic work; what the split-precision products execute on top is reported separately
    class_alg = r["launches"] / 2 * r["alg_flops_per_launch"] * 1e-12            # 2 instrumented steps in the record
    assert abs(class_alg - r["class_alg_tflop_per_step"]) / class_alg < 1e-3 and class_alg <= r["step_alg_tflop"]
    assert r["executed_tflop_per_step"] >= r["class_alg_tflop_per_step"] and 72.5 < r["class_alg_tflop_per_step"] < 73.8
    assert abs(r["achieved"] - r["class_alg_tflop_per_step"] / (d["kernels"]["gemm_bf16"]["ms_per_step"] * 1e-3)) / r["achieved"] < 1e-2
    # whole-step utilisation: algorithmic flops of the step over the step time
    assert abs(r["step_frac"] - r["step_alg_tflop"] / (d["ms_per_step"] * 1e-3) / r["peak"]) < 1e-3 and 74.0 < r["step_alg_tflop"] < 76.0
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample", "cpu_model", "encode_images_per_s", "fuse_rank_queries_per_s"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["unit"] == d["unit"] and c["cores"] >= 1
    # BASELINE.json's metric names Recall@K: the line carries it by default (round 5), against the scores the UNMODIFIED REFERENCE produced for
    # every 22nd query of the planted CIRR-val-sized case, on fp32-valued and on fp16-valued trunk weights (tests/golden/planted_c2_subset_eva*.npz)
    rc = d["recall"]
    assert rc["equal_recall_at_1_5_10"] is True and "REFERENCE" in rc["case"]
    for key in ("fp32_weights", "fp16_valued_trunk"):
        sub = rc[key]
        assert sub["scores"] == 191 * 2297 and sub["equal_recall_at_1_5_10"] and sub["equal_subset_recalls"] and sub["top1_image_equal_pct"] == 100.0
        assert sub["engine"]["recall_at_10"] == sub["reference"]["recall_at_10"] > 20.0
        assert abs(sub["engine"]["recall_at_50"] - sub["reference"]["recall_at_50"]) < 0.6 and sub["rms_dsim"] < 3e-4      # one query of 191 = 0.52 points
    # (as measured in round 6: max 1.08e-3, 5 of 438 727 scores over 1e-3 -- the flat 1e-3 of this size is a distribution statement)
    assert rc["fp16_valued_trunk"]["max_abs_dsim"] < 1.2e-3 and rc["fp16_valued_trunk"]["scores_over_1e-3"] <= 10
    assert sorted(rc["fixtures_evaluated"]) == ["fp16_valued_trunk", "fp32_weights"]
    assert d["config"]["per_rank_ms_per_step"] == [d["ms_per_step"]]
    # config C5's per-GPU step rides along (round 6): ViT-L, fp8 MFMA, 20 timed steps by a second invocation
    x = d["extra"]["c5_per_gpu_step"]
    assert x["dtype"] == "fp8" and x["backbone"] == "pretrain_vitL" and x["steps"] == 20 and x["peak_tflops"] == 5000.0
    assert abs(x["value"] - 128.0 / (x["ms_per_step"] * 1e-3)) / x["value"] < 1e-3 and 0.1 < x["step_frac"] < 0.5


def test_committed_default_line_carries_the_power_reading():
    """`roofline.power` (round 6): rocm-smi socket power + shader clock over extra un-timed steps; the part sits near its 1400-W cap far below the
    2.4 GHz the 2.5 PF peak assumes -- profiles/r06_bench_default_line.json is an unedited `python bench.py --full` line."""
    d = json.loads((ROOT / "profiles" / "r06_bench_default_line.json").read_text())
    pw = d["roofline"]["power"]
    assert pw["samples"] >= 3 and 1000 < pw["socket_w_mean"] <= pw["socket_w_max"] <= 1450 and 1200 < pw["sclk_mhz_mean"] < 2400
    assert abs(pw["peak_at_sclk_tflops"] - 2500.0 * pw["sclk_mhz_mean"] / 2400.0) < 1.0
    assert d["roofline"]["step_frac"] < pw["step_frac_of_peak_at_sclk"] < 1.0
    for k in ("recall", "extra", "cpu_baseline"):
        assert k in d, k


def test_committed_rocprof_summary_agrees_with_the_bench_line():
    import csv
    d = json.loads((ROOT / "profiles" / "r06_bench_n1.json").read_text())
    rows = list(csv.DictReader((ROOT / "profiles" / "r06_bench_kernel_stats.csv").open()))
    gemm_ms = sum(float(r["TotalDurationNs"]) for r in rows if "gemm" in r["Name"] or "splitk" in r["Name"]) / 4e6   # 4 steps profiled
    ev = d["kernels"]["gemm_bf16"]["ms_per_step"]
    assert abs(gemm_ms - ev) / ev < 0.03, (gemm_ms, ev)


def test_committed_counter_summary_has_the_utilisation_numbers():
    d = json.loads((ROOT / "profiles" / "r06_pmc.json").read_text())
    g = d["classes"]["gemm_anti"]["derived"]
    for k in ("mfma_busy_frac", "mfma_busy_frac_of_wall_at_2p4GHz", "effective_clock_GHz_upper_bound", "lds_bank_conflict_frac",
              "sq_wait_any_frac_of_wave_cycles", "hbm_side_GBs"):
        assert k in g and g[k] > 0, k
    assert 0.2 < g["mfma_busy_frac_of_wall_at_2p4GHz"] <= g["mfma_busy_frac"] < 1.0 and 1.0 < g["effective_clock_GHz_upper_bound"] < 2.45
    # the clock ratio is only formed for long dispatches (it read 3.3 GHz on 12-us launches)
    assert "effective_clock_GHz_upper_bound" not in d["classes"]["gemm_128"]["derived"]
    t = json.loads((ROOT / "profiles" / "r06_traffic.json").read_text())
    b = json.loads((ROOT / "profiles" / "r06_bench_n1.json").read_text())
    per_launch = t["gemm_bytes_per_step"]["total"] / b["kernels"]["gemm_bf16"]["launches_per_step"]
    assert abs(per_launch - b["roofline"]["traffic"]) / per_launch < 1e-3
    assert t["kernel_source_sha"][:12] in b["roofline"]["traffic_source"]


def test_fp8_bench_line_is_priced_against_the_fp8_peak():
    d = json.loads((ROOT / "profiles" / "r06_bench_vitL_fp8.json").read_text())
    assert d["dtype"] == "fp8" and d["roofline"]["peak"] == 5000.0
    b = json.loads((ROOT / "profiles" / "r06_bench_vitL_bf16.json").read_text())
    assert d["value"] > b["value"]
    c5 = json.loads((ROOT / "profiles" / "r06_bench_c5_slice_fp8.json").read_text())
    assert c5["config"]["shard"] == 125000 and c5["config"]["queries"] == 10000 and "EXTRAPOLATED" in c5["config"]["workload"]
    assert c5["steps"] >= 200                            # 200 timed encode steps behind the per-step figure, not 20
    t = c5["config"]["shard"] / c5["config"]["batch"] * c5["ms_per_step"] * 1e-3 + c5["config"]["fuse_rank_ms"] * 1e-3
    assert abs(c5["value"] - c5["config"]["shard"] / t) / c5["value"] < 1e-3


def test_same_box_dtype_comparison_is_on_record():
    """fp16 (headline) vs bf16 vs fp16 without the split-precision Q-Former, same box, same build: what parity costs."""
    f16, b16, single = (json.loads((ROOT / "profiles" / f"r06_bench_n1{t}.json").read_text()) for t in ("", "_bf16", "_fp16_single"))
    assert f16["dtype"] == "fp16" and b16["dtype"] == "bf16" and single["dtype"] == "fp16"
    assert b16["value"] > single["value"] > f16["value"] > 0.85 * b16["value"]


def test_bench_options_parse_without_a_gpu():
    """A plain run measures the headline only; --full adds the objects measured after the timed region; --dump-outputs DIR writes the last
    timed step's outputs; --steps sets the timed steps and must be positive.  Argument parsing needs no GPU."""
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in p.stdout, opt
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps" in p.stderr
