#!/usr/bin/env python3
"""`python -m sprc_amd.blip_fine_tune_2 --dataset CIRR|fashionIQ --blip-model-name blip2_cir_align_prompt --model-path X ...`

The reference's fine-tuning script (src/blip_fine_tune_2.py: clip_finetune_cirr :196-354, clip_finetune_fiq :25-192) on the HIP
training step: the same arguments and defaults (:370-391), AdamW (0.9, 0.98) / eps 1e-7 / weight decay 0.05 under torch's OneCycleLR,
GradScaler, the same `train_metrics.csv` / `validation_metrics.csv` / `training_hyperparameters.json` / `saved_models/*.pt`, with the
per-epoch validation of sprc_amd/harness.py.  The parameter update is sprc_amd.optim.FusedAdamW (one HIP launch per step).

Beyond the reference: --model-path (initial weights; nothing can be downloaded), --train-products, --dtype, --optimizer, --seed,
--max-steps, --vit-depth, --dress-types, and --resume DIR: every epoch also writes `saved_models/training_state.pt` (model,
optimiser, scaler, scheduler, counters, RNG states), from which an interrupted run continues in its directory.
Checkpoints: with --save-training, `--save-best` keeps the best epoch only (`tuned_clip_arithmetic` for CIRR by the arithmetic mean,
`tuned_clip_best` for FashionIQ by average_recall), as the reference's script does; without --save-best the reference's script saves
nothing at all -- here every validated epoch is then saved as `tuned_clip_{epoch}`.
Not here: the squarepad transform, the stage-2 (rerank) objective, multi-GPU training.
"""
from __future__ import annotations

import csv
import json
import os
import random
from argparse import ArgumentParser
from datetime import datetime
from pathlib import Path
from statistics import harmonic_mean, mean

import numpy as np
import torch
from torch.optim.lr_scheduler import OneCycleLR
from torch.utils.data import DataLoader

from .processors import generate_randomized_fiq_caption

CIRR_SCHEDULE_EPOCHS = 80             # blip_fine_tune_2.py:260: the CIRR schedule spans 80 epochs whatever --num-epochs says
ADAMW = dict(betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)        # :257-259, :90-93
CIRR_COLUMNS = ["group_recall_at1", "group_recall_at2", "group_recall_at3", "recall_at1", "recall_at5", "recall_at10", "recall_at50",
                "mean(R@5+R_s@1)", "arithmetic_mean", "harmonic_mean", "geometric_mean"]


def build_parser() -> ArgumentParser:
    p = ArgumentParser()
    # the reference's arguments and defaults (:370-391)
    p.add_argument("--dataset", type=str, required=True, help="should be either 'CIRR' or 'fashionIQ'")
    p.add_argument("--data-path", type=str, default="./cirr_dataset")
    p.add_argument("--num-workers", type=int, default=2)
    p.add_argument("--num-epochs", default=300, type=int, help="number training epochs")
    p.add_argument("--blip-model-name", default="blip2_cir_cat", type=str,
                   help="the reference's default names a model it does not ship: pass blip2_cir_align_prompt")
    p.add_argument("--backbone", type=str, default="pretrain", help="pretrain for vit-g, pretrain_vitL for vit-l")
    p.add_argument("--learning-rate", default=2e-6, type=float, help="Learning rate")
    p.add_argument("--batch-size", default=512, type=int, help="Batch size")
    p.add_argument("--loss-align", default=0.4, type=float)
    p.add_argument("--loss-rtc", default=0.4, type=float)
    p.add_argument("--loss-itm", default=1, type=float)
    p.add_argument("--validation-frequency", default=1, type=int, help="Validation frequency expressed in epochs")
    p.add_argument("--target-ratio", default=1.25, type=float, help="TargetPad target ratio")
    p.add_argument("--transform", default="targetpad", type=str, help="Preprocess pipeline: 'targetpad' ('squarepad' is not built)")
    p.add_argument("--save-training", dest="save_training", action="store_true", help="Whether save the training model")
    p.add_argument("--save-best", dest="save_best", action="store_true", help="Save only the best model during training")
    p.add_argument("--save-memory", dest="save_memory", action="store_true")
    # beyond the reference
    p.add_argument("--model-path", type=str, default=None, help="initial weights: {ClassName: state_dict}, as blip_validate reads them")
    p.add_argument("--train-products", default="fp16", choices=["fp16", "fp32"],
                   help="fp16 (default): fp16 operand copies + fp16 frozen trunk, the reference's autocast arithmetic; fp32: the parity mode")
    p.add_argument("--dtype", default="fp16", choices=["bf16", "fp16", "fp32"], help="engine of the per-epoch validation (blip_validate's --dtype)")
    p.add_argument("--optimizer", default="fused", choices=["fused", "torch"], help="fused: sprc_amd.optim.FusedAdamW; torch: torch.optim.AdamW")
    p.add_argument("--seed", type=int, default=None, help="seeds Python's / numpy's / torch's generators and the dropout masks")
    p.add_argument("--max-steps", type=int, default=None, help="stop after N optimiser steps of this invocation (the epoch in progress is closed)")
    p.add_argument("--vit-depth", type=int, default=None, help="truncate the ViT to N blocks (entry-point smoke tests only)")
    p.add_argument("--dress-types", nargs="+", default=["dress", "toptee", "shirt"], help="fashionIQ: categories trained and validated on")
    p.add_argument("--resume", type=str, default=None, help="run directory to continue (reads saved_models/training_state.pt)")
    return p


def hyper_params(a) -> dict:
    """The dictionary the reference writes to training_hyperparameters.json (:397-414)."""
    return {"num_epochs": a.num_epochs, "num_workers": a.num_workers, "blip_model_name": a.blip_model_name, "backbone": a.backbone,
            "learning_rate": a.learning_rate, "batch_size": a.batch_size, "validation_frequency": a.validation_frequency,
            "transform": a.transform, "target_ratio": a.target_ratio, "save_training": a.save_training, "save_best": a.save_best,
            "data_path": a.data_path, "loss_rtc": a.loss_rtc, "loss_align": a.loss_align, "loss_itm": a.loss_itm,
            "save_memory": a.save_memory}


def check_args(a) -> str:
    """-> 'cirr' | 'fashioniq'; refuses what cannot run BEFORE anything is loaded."""
    ds = a.dataset.lower()
    if ds not in ("fashioniq", "cirr"):
        raise ValueError("Dataset should be either 'CIRR' or 'FashionIQ")
    if ds == "cirr" and a.num_epochs > CIRR_SCHEDULE_EPOCHS:
        raise SystemExit(f"blip_fine_tune_2: --num-epochs {a.num_epochs} > {CIRR_SCHEDULE_EPOCHS}: the CIRR learning-rate schedule is "
                         f"OneCycleLR(..., epochs={CIRR_SCHEDULE_EPOCHS}) whatever --num-epochs says (blip_fine_tune_2.py:260); it has "
                         f"no step after epoch {CIRR_SCHEDULE_EPOCHS} and the reference's run dies there")
    if ds == "fashioniq" and a.num_epochs < 2:
        raise SystemExit(f"blip_fine_tune_2: --num-epochs {a.num_epochs}: the FashionIQ schedule is OneCycleLR(pct_start=1.5 / num_epochs, ...) "
                         "(blip_fine_tune_2.py:95), which needs at least 2 epochs; use --max-steps to stop a run early")
    if a.transform != "targetpad":
        raise SystemExit(f"blip_fine_tune_2: --transform {a.transform}: only 'targetpad' is built (the reference's scripts use no other)")
    if a.num_epochs < 1 or a.batch_size < 1 or a.validation_frequency < 1:
        raise SystemExit("blip_fine_tune_2: --num-epochs, --batch-size and --validation-frequency must be >= 1")
    return ds


def build_scheduler(optimizer, dataset: str, learning_rate: float, steps_per_epoch: int, num_epochs: int) -> OneCycleLR:
    """torch's own OneCycleLR with the reference's arguments: CIRR :260, FashionIQ :95."""
    if dataset == "cirr":
        return OneCycleLR(optimizer, max_lr=learning_rate, pct_start=1 / 50, steps_per_epoch=steps_per_epoch, epochs=CIRR_SCHEDULE_EPOCHS)
    return OneCycleLR(optimizer, max_lr=learning_rate, pct_start=1.5 / num_epochs, div_factor=100., steps_per_epoch=steps_per_epoch,
                      epochs=num_epochs)


def build_optimizer(kind: str, model, learning_rate: float):
    groups = [{"params": [p for p in model.parameters() if p.requires_grad], "lr": learning_rate, **ADAMW}]
    if kind == "fused":
        from .optim import FusedAdamW
        return FusedAdamW(groups)
    return torch.optim.AdamW(groups)


def append_csv_row(path: Path, row: dict) -> None:
    """One row at the end of `path`; the header is written when the file is new (the reference rewrites the whole frame each
    epoch -- the same file, but a resumed run has no frame to rewrite)."""
    path = Path(path)
    new = not path.exists() or path.stat().st_size == 0
    if not new:
        with open(path, newline="") as f:
            header = next(csv.reader(f))
        if header != list(row):
            raise ValueError(f"{path}: columns {header} differ from this row's {list(row)}")
    with open(path, "a", newline="") as f:
        w = csv.DictWriter(f, fieldnames=list(row))
        if new:
            w.writeheader()
        w.writerow(row)


def save_model(name: str, cur_epoch: int, model_to_save, training_path: Path) -> Path:
    """utils.py:208-222: {'epoch': e, ClassName: state_dict} under <run>/saved_models/<name>.pt."""
    models_path = Path(training_path) / "saved_models"
    models_path.mkdir(exist_ok=True, parents=True)
    out = models_path / f"{name}.pt"
    torch.save({"epoch": cur_epoch, model_to_save.__class__.__name__: model_to_save.state_dict()}, str(out))
    return out


def set_seed(seed: int) -> None:
    random.seed(seed)
    np.random.seed(seed % 2 ** 32)
    torch.manual_seed(seed)


def _load_model(a, device):
    from .model import load_model_and_preprocess
    kw = dict(compute_dtype=a.dtype, train_products=a.train_products, train_vit_dtype="fp16" if a.train_products == "fp16" else "fp32",
              max_batch=max(128, a.batch_size))
    if a.vit_depth is not None:
        from .config import get_config
        kw["cfg"] = get_config(a.backbone, vit_depth=a.vit_depth)
    model, _, txt = load_model_and_preprocess(name=a.blip_model_name, model_type=a.backbone, is_eval=False, device=device, **kw)
    return model, txt


def _cirr_results(results) -> dict:
    from .blip_validate import _geometric_mean
    g1, g2, g3, r1, r5, r10, r50 = results
    vals = [g1, g2, g3, r1, r5, r10, r50, (g1 + r5) / 2, mean(results), harmonic_mean(results), _geometric_mean(results)]
    return dict(zip(CIRR_COLUMNS, vals))                              # :330-342


def _fiq_results(dress_types, r10s, r50s) -> dict:
    out = {}
    for d, a, b in zip(dress_types, r10s, r50s):
        out[f"{d}_recall_at10"], out[f"{d}_recall_at50"] = a, b
    out.update({"average_recall_at10": mean(r10s), "average_recall_at50": mean(r50s), "average_recall": (mean(r50s) + mean(r10s)) / 2})
    return out                                                        # :171-179


def fine_tune(a, on_step=None) -> Path:
    """Both loops of the reference (they differ in the datasets, the caption handling, the loss weights, the schedule and the
    validation); -> the run directory.  on_step: called before every forward pass with a dict of the loop's objects (epoch,
    global_step, model, optimizer, scaler, scheduler, raw_captions, captions) -- for progress reporting and tests."""
    ds = check_args(a)
    from . import data_utils as du
    from .harness import collate_fn, compute_cirr_val_metrics, compute_fiq_val_metrics, extract_index_blip_features
    tag = "cirr" if ds == "cirr" else "fiq"
    state = None
    if a.resume:
        training_path = Path(a.resume)
        state_path = training_path / "saved_models" / "training_state.pt"
        if not state_path.exists():
            raise SystemExit(f"blip_fine_tune_2: --resume {training_path}: {state_path} does not exist")
        state = torch.load(state_path, map_location="cpu", weights_only=False)
        for k, want in (("dataset", ds), ("blip_model_name", a.blip_model_name), ("backbone", a.backbone), ("batch_size", a.batch_size)):
            if state[k] != want:
                raise SystemExit(f"blip_fine_tune_2: --resume: the run in {training_path} has {k} = {state[k]!r}, this call {want!r}")
        if ds != "cirr" and state["num_epochs"] != a.num_epochs:
            raise SystemExit(f"blip_fine_tune_2: --resume: the FashionIQ schedule spans --num-epochs (here {state['num_epochs']}); "
                             f"continue with the same value, not {a.num_epochs}")
    else:
        if not a.model_path:
            raise SystemExit("blip_fine_tune_2: --model-path is required (the reference downloads the pretrained BLIP-2 weights; "
                             "nothing is downloaded here)")
        start = datetime.now().strftime("%Y-%m-%d_%H:%M:%S")
        training_path = Path(du.base_path / f"models/clip_finetuned_on_{tag}_{a.blip_model_name}_{start}")
        training_path.mkdir(exist_ok=False, parents=True)
        with open(training_path / "training_hyperparameters.json", "w+") as f:
            json.dump(hyper_params(a), f, sort_keys=True, indent=4)
    if a.seed is not None:
        set_seed(a.seed)

    from .blip_validate import _device
    device = _device()
    model, txt_processors = _load_model(a, device)
    if state is not None:
        model.load_state_dict(state["model"], strict=False)
    else:
        ckpt = torch.load(a.model_path, map_location=device)
        msg = model.load_state_dict(ckpt[model.__class__.__name__], strict=False)
        print("Missing keys {}".format(msg.missing_keys))
    if a.seed is not None:
        model.dropout_seed = a.seed

    preprocess = du.targetpad_transform(a.target_ratio, 224)
    print(f"Target pad with target_ratio = {a.target_ratio} preprocess pipeline is used")
    if ds == "cirr":
        relative_val, classic_val = [du.CIRRDataset("val", "relative", preprocess)], [du.CIRRDataset("val", "classic", preprocess)]
        relative_train = du.CIRRDataset("train", "relative", preprocess)
    else:
        relative_val = [du.FashionIQDataset("val", [d], "relative", preprocess) for d in a.dress_types]
        classic_val = [du.FashionIQDataset("val", [d], "classic", preprocess) for d in a.dress_types]
        relative_train = du.FashionIQDataset("train", list(a.dress_types), "relative", preprocess)
    ctx = (os.environ.get("SPRC_LOADER_CONTEXT") or "forkserver") if a.num_workers > 0 else None
    train_loader = DataLoader(dataset=relative_train, batch_size=a.batch_size, num_workers=a.num_workers, pin_memory=False,
                              collate_fn=collate_fn, drop_last=True, shuffle=True, multiprocessing_context=ctx)
    if len(train_loader) == 0:
        raise SystemExit(f"blip_fine_tune_2: {len(relative_train)} training triplets give no batch of {a.batch_size} (drop_last)")

    optimizer = build_optimizer(a.optimizer, model, a.learning_rate)
    scheduler = build_scheduler(optimizer, ds, a.learning_rate, len(train_loader), a.num_epochs)
    scaler = torch.amp.GradScaler("cuda")
    best = {"arithmetic_mean": 0, "average_recall": 0}
    first_epoch, global_step = 0, 0
    if state is not None:
        optimizer.load_state_dict(state["optimizer"])
        scheduler.load_state_dict(state["scheduler"])
        scaler.load_state_dict(state["scaler"])
        best, first_epoch, global_step = state["best"], state["epoch"] + 1, state["global_step"]
        model._drop_step, model.dropout_seed = state["drop_step"], state["dropout_seed"]
        random.setstate(state["rng"]["python"])
        np.random.set_state(state["rng"]["numpy"])
        torch.set_rng_state(state["rng"]["torch"])
        print(f"resumed {training_path} after epoch {state['epoch']} ({global_step} optimiser steps)")
    loss_weights = {"loss_rtc": a.loss_rtc, "loss_align": a.loss_align, "loss_itm": a.loss_itm}

    print("Training loop started")
    steps_here, stop = 0, False
    for epoch in range(first_epoch, a.num_epochs):
        running = {"images_in_epoch": 0}
        for reference_images, target_images, captions in train_loader:
            images_in_batch = reference_images.size(0)
            optimizer.zero_grad()
            reference_images = reference_images.to(device, non_blocking=True)
            target_images = target_images.to(device, non_blocking=True)
            raw_captions = captions
            if ds != "cirr":                                           # (a) cap1 and cap2 (b) cap2 and cap1 (c) cap1 (d) cap2   (:122-124)
                captions = generate_randomized_fiq_caption(np.array(captions).T.flatten().tolist())
            captions = [txt_processors["eval"](c) for c in captions]
            if on_step is not None:
                on_step(dict(epoch=epoch, global_step=global_step, model=model, optimizer=optimizer, scaler=scaler, scheduler=scheduler,
                             raw_captions=raw_captions, captions=captions))
            model.train()
            with torch.amp.autocast("cuda"):
                try:
                    loss_dict = model({"image": reference_images, "target": target_images, "text_input": captions})
                except NotImplementedError as e:                       # the rerank class: its stage-2 objective is not built
                    raise SystemExit(f"blip_fine_tune_2: {e}")
                loss = 0.
                for key in loss_dict.keys():
                    if ds == "cirr" and key != "loss_itc":
                        loss += loss_weights[key] * loss_dict[key]     # :293-299
                    else:
                        loss += loss_dict[key]                         # :129-132
            scaler.scale(loss).backward()
            scaler.step(optimizer)
            scaler.update()
            scheduler.step()
            # update_train_running_results_dict (utils.py:176-188): image-weighted sums, one read of the three losses per step
            values = torch.stack([loss_dict[k].detach() for k in loss_dict]).tolist()
            for k, v in zip(loss_dict, values):
                running[k] = running.get(k, 0) + v * images_in_batch
            running["images_in_epoch"] += images_in_batch
            global_step += 1
            steps_here += 1
            if a.max_steps is not None and steps_here >= a.max_steps:
                stop = True
                break

        row = {"epoch": epoch}
        row.update({k: float(v / running["images_in_epoch"]) for k, v in running.items() if k != "images_in_epoch"})
        append_csv_row(training_path / "train_metrics.csv", row)

        if epoch % a.validation_frequency == 0:
            model.eval()
            if ds == "cirr":
                feats, names = extract_index_blip_features(classic_val[0], model, num_workers=a.num_workers)
                results_dict = _cirr_results(compute_cirr_val_metrics(relative_val[0], model, feats, names, txt_processors))
                metric, best_name = "arithmetic_mean", "tuned_clip_arithmetic"
            else:
                r10s, r50s = [], []
                for rel, cla in zip(relative_val, classic_val):
                    feats, names = extract_index_blip_features(cla, model, a.save_memory, num_workers=a.num_workers)
                    r10, r50 = compute_fiq_val_metrics(rel, model, feats, names, txt_processors, a.save_memory)
                    r10s.append(r10)
                    r50s.append(r50)
                    torch.cuda.empty_cache()
                results_dict = _fiq_results(a.dress_types, r10s, r50s)
                metric, best_name = "average_recall", "tuned_clip_best"
            del feats
            print(json.dumps(results_dict, indent=4))
            log = {"epoch": epoch}
            log.update(results_dict)
            append_csv_row(training_path / "validation_metrics.csv", log)
            if a.save_training:
                if not a.save_best:
                    save_model(f"tuned_clip_{epoch}", epoch, model, training_path)
                elif results_dict[metric] > best[metric]:
                    best[metric] = results_dict[metric]
                    save_model(best_name, epoch, model, training_path)

        (training_path / "saved_models").mkdir(exist_ok=True, parents=True)
        tmp = training_path / "saved_models" / "training_state.pt.tmp"
        torch.save({"dataset": ds, "blip_model_name": a.blip_model_name, "backbone": a.backbone, "batch_size": a.batch_size,
                    "num_epochs": a.num_epochs, "epoch": epoch, "global_step": global_step, "model": model.state_dict(),
                    "optimizer": optimizer.state_dict(), "scaler": scaler.state_dict(), "scheduler": scheduler.state_dict(),
                    "drop_step": model._drop_step, "dropout_seed": model.dropout_seed, "best": best,
                    "rng": {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state()}}, str(tmp))
        os.replace(tmp, training_path / "saved_models" / "training_state.pt")
        if stop:
            print(f"--max-steps {a.max_steps} reached in epoch {epoch}")
            break
    return training_path


def main(argv=None, on_step=None) -> Path:
    return fine_tune(build_parser().parse_args(argv), on_step=on_step)


if __name__ == "__main__":
    main()
