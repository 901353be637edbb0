"""End-to-end GPU parity of the composite forward passes against REFERENCE-generated goldens
(tests/golden/*.npz, produced by running the unmodified reference; see oracle/gen_golden.py).

fp32 engine ("parity mode", exact fp32 MFMA): cosine scores within 1e-3 is the north-star bar; we hold
1e-4.  bf16 engine (the throughput mode): measured deviation is asserted against the same 1e-3 bar on
the similarity scores and printed for DESIGN.md.
"""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu

from oracle import sprc_oracle as O  # noqa: E402
from sprc_amd import engine as E  # noqa: E402
from sprc_amd import synth  # noqa: E402
from sprc_amd.config import get_config  # noqa: E402

DEV = "cuda:0"

import sys as _sys, os as _os  # noqa: E402
_sys.path.insert(0, _os.path.dirname(_os.path.abspath(__file__)))
import _cases as CASES  # noqa: E402  (session-lived full-depth state dicts: tests/_cases.py)


def _setup(golden_dir, name, dtype):
    g = np.load(golden_dir / name, allow_pickle=False)
    cfg = get_config(str(g["model_type"]), vit_depth=int(g["vit_depth"]))
    sd = CASES.state_dict(cfg, int(g["seed"]))
    images = synth.make_images(int(g["n_img"]), seed=int(g["seed"]))
    np.testing.assert_array_equal(images[:, :, 0, :4].numpy(), g["image_probe"])
    eng = E.Engine(cfg, sd, DEV, dtype=dtype, max_batch=8)
    return g, cfg, eng, images


def _run(g, eng, images):
    raw = eng.vit_forward(images.to(DEV))
    feats, _ = eng.qformer_image(raw)
    ref = torch.from_numpy(g["ref_index"]).to(DEV)
    fusion, _ = eng.qformer_fuse(raw[ref], torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"]))
    sim = E.sim_max(fusion, feats)
    torch.cuda.synchronize()
    return raw.cpu().numpy(), feats.cpu().numpy(), fusion.cpu().numpy(), sim.cpu().numpy()


@pytest.mark.parametrize("name", ["tiny_eva.npz", "tiny_clip.npz", "full_eva.npz", "full_clip.npz"])
def test_fp32_engine_matches_reference(golden_dir, name):
    g, cfg, eng, images = _setup(golden_dir, name, "fp32")
    raw, feats, fusion, sim = _run(g, eng, images)
    rows = g["rows"].tolist()
    deep = int(g["vit_depth"]) > 8
    np.testing.assert_allclose(raw[:, rows], g["raw"], atol=2e-3 if deep else 2e-4, rtol=0)
    np.testing.assert_allclose(feats, g["feats"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(np.linalg.norm(feats, axis=-1), 1.0, atol=1e-5)
    np.testing.assert_allclose(fusion, g["fusion"], atol=1e-4, rtol=0)
    np.testing.assert_allclose(sim, g["sim"], atol=1e-4, rtol=0)          # bar: 1e-3
    print(f"\n[{name} fp32] max|dsim|={np.abs(sim - g['sim']).max():.2e} max|dfeats|={np.abs(feats - g['feats']).max():.2e} "
          f"max|draw|={np.abs(raw[:, rows] - g['raw']).max():.2e}")


@pytest.mark.parametrize("name", ["tiny_eva.npz", "tiny_clip.npz", "full_eva.npz", "full_clip.npz"])
def test_bf16_engine_within_tolerance(golden_dir, name):
    g, cfg, eng, images = _setup(golden_dir, name, "bf16")
    raw, feats, fusion, sim = _run(g, eng, images)
    rows = g["rows"].tolist()
    dsim = np.abs(sim - g["sim"]).max()
    cos_feats = (feats * g["feats"]).sum(-1).min()
    cos_fusion = (fusion * g["fusion"]).sum(-1).min()
    print(f"\n[{name} bf16] max|dsim|={dsim:.2e} min cos(feats)={cos_feats:.6f} min cos(fusion)={cos_fusion:.6f} "
          f"max|draw|={np.abs(raw[:, rows] - g['raw']).max():.2e}")
    assert cos_feats > 0.995 and cos_fusion > 0.995
    assert dsim < 1e-3        # the north star's tolerance: cosine scores within 1e-3 of the fp32 CPU path (measured 4e-4 .. 8e-4)


def test_ranking_is_bit_exact_on_device_scores(golden_dir):
    """indices: HIP top-k / rank_of on the HIP scores == oracle stable order of the SAME scores (integer work,
    bit-exact), and == the order of the reference's own scores wherever those are not within fp32 noise of a tie."""
    g, cfg, eng, images = _setup(golden_dir, "tiny_eva.npz", "fp32")
    _, _, _, sim = _run(g, eng, images)
    d = torch.from_numpy(sim).to(DEV)
    k = min(64, sim.shape[1])
    _, idx = E.topk(d, k)
    np.testing.assert_array_equal(idx.cpu().numpy()[:, :sim.shape[1]], O.rank_stable(sim)[:, :k].astype(np.int32))
    ref_order = O.rank_stable(g["sim"])
    gap = np.abs(np.diff(np.take_along_axis(g["sim"], ref_order, axis=1), axis=1)).min()
    if gap > 1e-4:
        np.testing.assert_array_equal(idx.cpu().numpy()[:, :sim.shape[1]], ref_order[:, :k].astype(np.int32))


def test_two_stream_vit_matches_single_stream(tmp_path):
    """SPRC_VIT_STREAMS=2 pipelines the two halves of a batch on two streams inside sprc_vit_forward (read once per
    process, hence the subprocesses).  Rows are independent, so the result must not change: identical bits here (both
    modes use the same GEMM kernels at this size), and the Q-Former features computed from it agree likewise."""
    import subprocess
    import sys
    script = (
        "import sys, numpy as np, torch\n"
        "from sprc_amd import engine as E, synth\n"
        "from sprc_amd.config import get_config\n"
        "cfg = get_config('pretrain', vit_depth=3)\n"
        "sd = synth.make_state_dict(cfg, seed=5)\n"
        "eng = E.Engine(cfg, sd, 'cuda:0', dtype='bf16', max_batch=20)\n"
        "raw = eng.vit_forward(synth.make_images(20, seed=6).to('cuda:0'))\n"
        "feats, _ = eng.qformer_image(raw)\n"
        "torch.cuda.synchronize()\n"
        "np.savez(sys.argv[1], raw=raw.cpu().numpy(), feats=feats.cpu().numpy())\n")
    out = {}
    for n in ("1", "2"):
        path = tmp_path / f"s{n}.npz"
        env = dict(os.environ, SPRC_VIT_STREAMS=n)
        subprocess.run([sys.executable, "-c", script, str(path)], check=True, env=env, cwd=str(ROOT), timeout=600)
        out[n] = np.load(path)
    assert np.isfinite(out["2"]["raw"]).all()
    np.testing.assert_array_equal(out["1"]["raw"], out["2"]["raw"])
    np.testing.assert_array_equal(out["1"]["feats"], out["2"]["feats"])


@pytest.mark.parametrize("q_layers", [12, 3, 1])
@pytest.mark.parametrize("model_type", ["pretrain", "pretrain_vitL"])
def test_ragged_batches_against_the_oracle(model_type, q_layers):
    """Composite entry points at batch sizes nobody padded for (1, 3, 5 images; 1, 2, 7 queries; captions of every length
    from 2 to 32 tokens) on a depth-1 backbone + the full Q-Former: fp32 engine vs the CPU oracle, and one engine sized
    for the largest batch reused for all of them (workspace carving, row maps of the text rows, masks).
    q_layers 3 and 1 (one batch each): with an odd count the LAST layer, which the fusion's first pass runs on its query
    rows alone, has cross-attention; in the 12-layer Q-Former it has none.  Same tolerances: fewer layers accumulate less error."""
    cfg = get_config(model_type, vit_depth=1, q_layers=q_layers)
    sd = synth.make_state_dict(cfg, seed=21)
    eng = E.Engine(cfg, sd, DEV, dtype="fp32", max_batch=8)
    for n_img, nq in ((1, 1), (3, 2), (5, 7)) if q_layers == 12 else ((3, 2),):
        images = synth.make_images(n_img, seed=30 + n_img)
        ids, mask, ref = synth.make_queries(nq, n_img, seed=40 + nq)
        for j in range(nq):                                  # caption lengths 2 .. 32 incl. the extremes
            L = [2, 32, 3, 17, 31, 9, 5][j % 7]
            ids[j, L - 1], ids[j, L:], mask[j, :L], mask[j, L:] = 102, 0, 1, 0
        with torch.no_grad():
            feats_o, raw_o = O.extract_target_features(sd, cfg, images)
            sim_o = O.inference(sd, cfg, raw_o[ref], feats_o, ids, mask).numpy()
        raw = eng.vit_forward(images.to(DEV))
        feats, _ = eng.qformer_image(raw)
        fusion, _ = eng.qformer_fuse(raw[ref.to(DEV)], ids, mask)
        sim = E.sim_max(fusion, feats).cpu().numpy()
        np.testing.assert_allclose(raw.cpu().numpy(), raw_o.numpy(), atol=2e-4, rtol=0)
        np.testing.assert_allclose(feats.cpu().numpy(), feats_o.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(sim.reshape(nq, n_img), sim_o.reshape(nq, n_img), atol=2e-5, rtol=0)
