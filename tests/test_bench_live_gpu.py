"""The driver's contract on a LIVE run: `python bench.py --gpus 1 --steps K --warmup W` prints ONE JSON line with BASELINE.json's metric
on its config, whole-job value consistent with the step time and the roofline object measured with HIP events inside the run; with
`--full` it also carries the objects measured after the timed region (recall, extra, roofline.power, and a cpu_baseline object when it
is not switched off); `--dump-outputs DIR` writes what the last timed step computed."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _run(*args, **extra_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_live_bench_line():
    base = json.loads((ROOT / "BASELINE.json").read_text())
    d = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline")
    assert base["metric"].startswith(d["metric"]) and d["unit"] == "images/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["dtype"] == "fp16" and "model" not in d["config"] and "CIRR-val" in d["config"]["workload"] and d["config"]["batch"] == 128
    assert d["value"] == pytest.approx(128.0 / (d["ms_per_step"] * 1e-3), rel=1e-3) and 500 < d["value"] < 5000
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and r["peak"] == 2500.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"], abs=2e-4)
    assert 0.2 < r["frac"] < 0.6 and 0.2 < r["step_frac"] < 0.6 and r["launches"] > 300 and r["avg_launch_ms"] > 0.05
    assert r["step_frac"] == pytest.approx(r["step_alg_tflop"] / (d["ms_per_step"] * 1e-3) / r["peak"], rel=2e-3)
    assert "cpu_baseline" not in d or d["cpu_baseline"] is None
    # the `recall` object of --full (BASELINE.json's metric names Recall@K): the engine against the reference-scored C2 subsets.  This is the
    # ONE live invocation that runs it (two more full-depth encodes of the 2297-image planted gallery: ~35 s); the others pass --no-recall
    rc = d["recall"]
    assert set(rc["fixtures_evaluated"]) == {"fp32_weights", "fp16_valued_trunk"} and rc["equal_recall_at_1_5_10"] is True
    assert rc["fp16_valued_trunk"]["rms_dsim"] < 2e-4 and rc["fp16_valued_trunk"]["scores_over_1e-3"] < 1e-3 * rc["fp16_valued_trunk"]["scores"]
    # roofline.power: rocm-smi over extra un-timed steps -- the part sits at its power cap, far below the 2.4 GHz the 2.5 PF peak assumes
    pw = r["power"]                       # (None where rocm-smi is missing or prints something else: the line must not depend on it)
    if pw is not None:
        assert pw["samples"] >= 3 and 800 < pw["socket_w_mean"] <= 1500 and 1000 < pw["sclk_mhz_mean"] < 2450
        assert pw["peak_at_sclk_tflops"] == pytest.approx(2500.0 * pw["sclk_mhz_mean"] / 2400.0, rel=1e-3) and r["step_frac"] < pw["step_frac_of_peak_at_sclk"] < 1.0
    else:
        print("\n[live bench line] roofline.power is null on this box (rocm-smi unavailable)")
    # the `extra` object of --full: config C5's per-GPU step (ViT-L, fp8 MFMA) measured by a second invocation
    x = d["extra"]["c5_per_gpu_step"]
    assert x["dtype"] == "fp8" and x["backbone"] == "pretrain_vitL" and x["steps"] == 20 and x["peak_tflops"] == 5000.0
    assert x["value"] == pytest.approx(128.0 / (x["ms_per_step"] * 1e-3), rel=1e-3) and 2000 < x["value"] < 12000 and 0.1 < x["step_frac"] < 0.5
    # a dtype the reference does not benchmark with is refused by argparse, not silently accepted
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--dtype", "int8"], cwd=ROOT, capture_output=True, text=True)
    assert p.returncode != 0


def test_plain_bench_line_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full the run only sets up, warms up, times the steps and prints the line: none of the objects measured after the timed
    region.  `--dump-outputs DIR` writes what the last timed step computed: its 233 queries' top-51 scores and gallery indices, their fused
    vectors, and the features of its 128 images, which that same step wrote into the resident gallery at slice `lo` and ranked against."""
    steps, warmup = 2, 1
    d = _run("--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path))
    assert d["steps"] == steps and d["warmup"] == warmup and d["dtype"] == "fp16" and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(128.0 / (d["ms_per_step"] * 1e-3), rel=1e-3) and 500 < d["value"] < 5000
    for k in ("recall", "extra", "cpu_baseline"):
        assert k not in d, k
    assert d["roofline"]["power"] is None
    out = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(out) == {"topk_scores", "topk_indices", "fusion", "image_feats"}
    assert all(x.dtype in (np.float32, np.float64) for x in out.values()) and sum(x.nbytes for x in out.values()) <= 64 << 20
    vals, idx, fusion, feats = out["topk_scores"], out["topk_indices"], out["fusion"], out["image_feats"]
    assert vals.shape == idx.shape == (233, 51) and fusion.shape == (233, 256) and feats.shape == (128, 32, 256)
    assert np.all(np.diff(vals, axis=1) <= 0) and np.all((idx >= 0) & (idx < 2297)) and np.all(idx == np.round(idx))
    np.testing.assert_allclose(np.linalg.norm(fusion, axis=1), 1.0, atol=1e-4)
    np.testing.assert_allclose(np.linalg.norm(feats, axis=2), 1.0, atol=1e-4)
    lo = ((warmup + steps - 1) * 128) % (2297 - 128)                       # bench.py: the gallery slice the last step's images replace
    sim = np.einsum("qe,nte->qnt", fusion.astype(np.float64), feats.astype(np.float64)).max(axis=2)      # [233, 128]: scores of that slice
    hit = (idx >= lo) & (idx < lo + 128)
    q, j = np.nonzero(hit)
    np.testing.assert_allclose(vals[q, j], sim[q, idx[q, j].astype(np.int64) - lo], atol=1e-4)
    listed = np.zeros(sim.shape, dtype=bool)
    listed[q, idx[q, j].astype(np.int64) - lo] = True
    assert np.all(sim[~listed] <= np.broadcast_to(vals[:, -1:], sim.shape)[~listed] + 1e-4)                 # the rest ranks below the top-51


def test_bench_line_through_a_one_rank_rccl_group():
    """The code `bench.py --gpus N` runs on an N-GPU node -- `init_process_group("nccl", device_id=...)`, the one-rank-per-device check, both
    device-side all_gathers of the sharded ranking, the per-rank step-time record, barrier + destroy -- executed on the 1-GPU box through a
    ONE-rank RCCL group (SPRC_BENCH_FORCE_DIST=1, SPRC_DIST_ALWAYS_EXCHANGE=1).  N > 1 itself stays unmeasured until a multi-GPU box runs it."""
    d = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-recall", "--no-power", SPRC_BENCH_FORCE_DIST="1", SPRC_DIST_ALWAYS_EXCHANGE="1")
    c = d["config"]
    assert c["rccl_ranks"] == 1 and c["backend"] == "rccl" and c["per_rank_ms_per_step"] == [d["ms_per_step"]]
    assert d["n_gpus"] == 1 and 500 < d["value"] < 5000


def test_bench_line_with_grouped_qformer_stage():
    """`--qf-group G`: the ViT runs per step, the Q-Former stage (gallery-side pass, fusion, ranking) once per G steps on their G x 128 images and
    G x 233 queries, a last partial group flushed inside the timed region: the line keeps the contract (value from the step time, per-step class
    figures from the instrumented group)."""
    d = _run("--gpus", "1", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-recall", "--no-power", "--qf-group", "2")
    assert d["config"]["qformer_group"] == 2 and d["steps"] == 5
    assert d["value"] == pytest.approx(128.0 / (d["ms_per_step"] * 1e-3), rel=1e-3) and 500 < d["value"] < 5000
    r = d["roofline"]
    assert 0.2 < r["frac"] < 0.6 and r["traffic"] is None                 # the committed counter profile belongs to the ungrouped command
    assert d["kernels"]["gemm_bf16"]["launches_per_step"] > 150


def test_bench_line_of_the_c5_slice():
    """Config C5's per-GPU share (synthetic 1 M-image gallery x 10 k composed queries, ViT-L backbone, fp8 MFMA, 8 GPUs): ONE GPU's
    125 000-image shard -- ViT-L encode steps on e4m3 operands timed live, then the shard's fusion and bf16 ranking passes at their real sizes
    (the full 1 M x 10 k ranking in 8 logical shards is tests/test_fullsize_gpu.py).  The 8-GPU run itself needs a multi-GPU box."""
    d = _run("--workload", "c5-slice", "--backbone", "pretrain_vitL", "--dtype", "fp8", "--steps", "20", "--warmup", "3")
    c = d["config"]
    assert d["dtype"] == "fp8" and c["backbone"] == "pretrain_vitL" and c["shard"] == 125000 and c["queries"] == 10000 and c["batch"] == 128
    assert d["steps"] == 20 and d["n_gpus"] == 1 and "C5 slice" in c["workload"] and c["rank_dtype"] == "bf16" and c["topk"] == 51
    assert 3000 < d["value"] < 12000 and 10 < d["ms_per_step"] < 45 and 20 < c["fuse_rank_ms"] < 500
    r = d["roofline"]
    assert r["peak"] == 5000.0 and 0.1 < r["frac"] < 0.5
