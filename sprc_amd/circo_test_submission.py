#!/usr/bin/env python3
"""`python -m sprc_amd.circo_test_submission --blip-model-name blip2_cir_align_prompt --model-path X [--circo-path P]`

CIRCO test submission file, in the manner of sprc_amd/cirr_test_submission.py (the reference has no CIRCO script):
`submission/CIRCO/<file>.json` = {query_id: [the ids of the first 50 gallery images]}.  The evaluation server's exact
format cannot be checked offline.
"""
from __future__ import annotations

import json
import os
from argparse import ArgumentParser

from .blip_validate import _load
from .harness import circo_reference_ids, extract_index_blip_features, generate_circo_test_dicts


def generate_circo_test_submissions(file_name: str, blip_model, preprocess, txt_processors, num_workers: int = 2, circo_path=None):
    from .data_utils import CIRCODataset, base_path
    root = circo_path or base_path / "CIRCO"
    classic = CIRCODataset(root, "test", "classic", preprocess)
    relative = CIRCODataset(root, "test", "relative", preprocess)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:                      # torchrun: gallery sharded over the ranks
        from .dist_eval import generate_circo_test_dicts_sharded
        top = generate_circo_test_dicts_sharded(relative, classic, blip_model, txt_processors, num_workers=num_workers)
        if int(os.environ.get("RANK", "0")) != 0:
            return
    else:
        # raw embeddings for the queries' reference images only: the gallery has 123 403 images
        feats, names = extract_index_blip_features(classic, blip_model, num_workers=num_workers, keep_raw=circo_reference_ids(relative))
        top = generate_circo_test_dicts(relative, blip_model, feats, names, txt_processors)
    folder = base_path / "submission" / "CIRCO"
    folder.mkdir(exist_ok=True, parents=True)
    print("Saving CIRCO test predictions")
    with open(folder / f"{file_name}.json", "w+") as f:
        json.dump(top, f, sort_keys=True)


def main(argv=None):
    from .blip_validate import _preprocess
    p = ArgumentParser()
    p.add_argument("--blip-model-name", default="blip2_cir_align_prompt", type=str)
    p.add_argument("--model-path", type=str)
    p.add_argument("--backbone", type=str, default="pretrain", help="pretrain for vit-g, pretrain_vitL for vit-l")
    p.add_argument("--circo-path", type=str, default=None, help="the dataset directory (default: <data root>/CIRCO)")
    p.add_argument("--dtype", default="fp16", choices=["bf16", "fp16", "fp32"])
    p.add_argument("--gpu-preprocess", action="store_true", help="image transform on the GPU (bit-identical to the PIL transform)")
    p.add_argument("--vit-depth", type=int, default=None, help="truncate the ViT to N blocks (entry-point smoke tests only)")
    a = p.parse_args(argv)
    model, txt = _load(a.blip_model_name, a.backbone, a.model_path, a.dtype, a.vit_depth)
    preprocess, workers = _preprocess(a.gpu_preprocess, model.device)
    generate_circo_test_submissions(f"circo_test_submission_{a.blip_model_name}", model, preprocess, txt, workers, a.circo_path)


if __name__ == "__main__":
    main()
