"""`python -m sprc_amd.blip_fine_tune_2` end to end on tiny datasets ON DISK (CIRR layout: 13 PNG files, train + val caption and
split files; FashionIQ layout: one category of 8 images), a depth-1 ViT, batches of 4: the artefacts of the reference's script
(training_hyperparameters.json, train_metrics.csv, validation_metrics.csv, saved_models/*.pt), the checkpoint through
sprc_amd.blip_validate, the FashionIQ caption randomiser inside the loop, and --resume (bookkeeping only: the two embedding-table
scatters of the backward use float atomics, so parameters are not bit-reproducible from run to run and are not compared)."""
import csv
import importlib
import json
import math
import os
import random
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))

from gen_preprocess_golden import synth_image  # noqa: E402
from sprc_amd import synth  # noqa: E402
from sprc_amd.config import get_config  # noqa: E402

N_IMG, N_TRAIN, N_VAL, DEPTH, BATCH = 13, 12, 7, 1, 4
WORDS = ["make", "the", "dog", "bigger", "remove", "person", "add", "a", "red", "hat", "and", "two", "cats", "instead", "of", "one",
         "brighter", "background", "is", "more", "colour", "##ful", "##s", "##er", "left", "right"]
MODEL = ["--blip-model-name", "blip2_cir_align_prompt", "--vit-depth", str(DEPTH), "--batch-size", str(BATCH), "--num-workers", "0"]
RECALLS = ["group_recall_at1", "group_recall_at2", "group_recall_at3", "recall_at1", "recall_at5", "recall_at10", "recall_at50"]


def _caption(rng):
    return " ".join(rng.choice(WORDS[:20], size=int(rng.integers(2, 7))).tolist())


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = tmp_path_factory.mktemp("sprc_finetune")
    cirr = root / "cirr_dataset" / "cirr"
    (cirr / "captions").mkdir(parents=True)
    (cirr / "image_splits").mkdir(parents=True)
    (root / "cirr_dataset" / "img").mkdir(parents=True)
    rng = np.random.default_rng(21)
    sizes = [(120, 90), (80, 150), (96, 96), (160, 60), (47, 101)]
    names = []
    for i in range(N_IMG):
        w, h = sizes[i % len(sizes)]
        name = f"img-{i:03d}"
        Image.fromarray(synth_image(w, h, 70 + i)).save(root / "cirr_dataset" / "img" / f"{name}.png")
        names.append(name)
    split = {n: f"img/{n}.png" for n in names}
    for sp, nq in (("train", N_TRAIN), ("val", N_VAL)):
        trip = []
        for q in range(nq):
            ref = int(rng.integers(0, N_IMG))
            tgt = int((ref + 1 + rng.integers(0, N_IMG - 1)) % N_IMG)
            others = [i for i in rng.permutation(N_IMG) if i not in (ref, tgt)][:4]
            members = [names[i] for i in rng.permutation([ref, tgt, *others])]
            trip.append({"pairid": 100 + q, "reference": names[ref], "target_hard": names[tgt], "caption": _caption(rng).capitalize() + ".",
                         "img_set": {"members": members}})
        (cirr / "captions" / f"cap.rc2.{sp}.json").write_text(json.dumps(trip))
        (cirr / "image_splits" / f"split.rc2.{sp}.json").write_text(json.dumps(split))
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + [".", ","]
    vocab += [f"tok{i}" for i in range(30522 - len(vocab))]
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    cfg = get_config("pretrain", vit_depth=DEPTH)
    sd = synth.make_state_dict(cfg, seed=23)
    torch.save({"Blip2QformerCirAlignPrompt": sd, "epoch": 0}, root / "ckpt.pt")
    os.environ["SPRC_DATA_ROOT"], os.environ["SPRC_BERT_VOCAB"] = str(root), str(root / "vocab.txt")
    import sprc_amd.data_utils as du
    importlib.reload(du)                                   # base_path is read at import
    return dict(root=root, sd=sd, ckpt=str(root / "ckpt.pt"))


@pytest.fixture(scope="module")
def fiq_world(world):
    """FashionIQ layout under the same root: one category, 8 images, 8 training and 5 validation triplets with two captions each."""
    fiq = world["root"] / "fashionIQ_dataset"
    for sub in ("captions", "image_splits", "images"):
        (fiq / sub).mkdir(parents=True, exist_ok=True)
    rng = np.random.default_rng(31)
    names = []
    for i in range(8):
        name = f"d{i:04d}"
        Image.fromarray(synth_image(90 + 13 * i, 140 - 7 * i, 500 + i)).save(fiq / "images" / f"{name}.png")
        names.append(name)
    edges = ["", ".", "?", ", ", " "]
    for sp, nq in (("train", 8), ("val", 5)):
        trip = []
        for q in range(nq):
            ref = int(rng.integers(0, 8))
            tgt = int((ref + 1 + rng.integers(0, 7)) % 8)
            trip.append({"candidate": names[ref], "target": names[tgt], "captions": [_caption(rng) + edges[(q + j) % len(edges)] for j in range(2)]})
        (fiq / "captions" / f"cap.dress.{sp}.json").write_text(json.dumps(trip))
        (fiq / "image_splits" / f"split.dress.{sp}.json").write_text(json.dumps(names))
    return world


def _rows(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def test_cirr_fine_tuning_end_to_end(world):
    from sprc_amd import blip_fine_tune_2 as ft
    from sprc_amd import blip_validate as bv
    run = ft.main(["--dataset", "CIRR", "--num-epochs", "2", "--max-steps", "6", "--validation-frequency", "1", "--save-training",
                   "--model-path", world["ckpt"], "--seed", "5", *MODEL])
    assert run.parent == world["root"] / "models" and run.name.startswith("clip_finetuned_on_cirr_blip2_cir_align_prompt_")
    hp = json.loads((run / "training_hyperparameters.json").read_text())
    assert hp["num_epochs"] == 2 and hp["batch_size"] == BATCH and hp["loss_rtc"] == 0.4 and hp["learning_rate"] == 2e-6
    train = _rows(run / "train_metrics.csv")
    assert [list(r) for r in train] == [["epoch", "loss_itc", "loss_rtc", "loss_align"]] * 2 and [r["epoch"] for r in train] == ["0", "1"]
    assert all(math.isfinite(float(v)) and float(v) > 0 for r in train for k, v in r.items() if k != "epoch")
    val = _rows(run / "validation_metrics.csv")
    assert len(val) == 2 and list(val[0]) == ["epoch", *RECALLS, "mean(R@5+R_s@1)", "arithmetic_mean", "harmonic_mean", "geometric_mean"]
    ckpt = run / "saved_models" / "tuned_clip_1.pt"
    assert ckpt.exists() and (run / "saved_models" / "tuned_clip_0.pt").exists() and (run / "saved_models" / "training_state.pt").exists()
    # what it saved is what it validated: the same seven recalls through the validation entry point
    out = bv.main(["--dataset", "CIRR", "--model-path", str(ckpt), "--vit-depth", str(DEPTH)])
    assert [out[k] for k in RECALLS] == [float(val[-1][k]) for k in RECALLS]
    assert float(val[-1]["arithmetic_mean"]) == pytest.approx(sum(out[k] for k in RECALLS) / 7)
    saved = torch.load(ckpt, map_location="cpu")
    assert saved["epoch"] == 1 and set(saved) == {"epoch", "Blip2QformerCirAlignPrompt"}
    tuned, sd = saved["Blip2QformerCirAlignPrompt"], world["sd"]
    q = "Qformer.bert.encoder.layer.0.attention.self.query.weight"
    assert not torch.equal(tuned[q], sd[q].float()) and torch.isfinite(tuned[q]).all()
    trunk = [k for k in sd if k.startswith("visual_encoder.")]
    assert trunk and all(torch.equal(tuned[k].float(), sd[k].float()) for k in trunk)


def test_fashioniq_fine_tuning_composes_the_randomised_captions(fiq_world):
    from sprc_amd import blip_fine_tune_2 as ft
    from sprc_amd.processors import BlipCaptionProcessor, generate_randomized_fiq_caption
    seen = []
    # one epoch (2 batches): the reference's schedule, pct_start = 1.5 / num_epochs, needs --num-epochs >= 2, so the run is stopped there
    run = ft.main(["--dataset", "fashionIQ", "--num-epochs", "2", "--max-steps", "2", "--dress-types", "dress", "--model-path", fiq_world["ckpt"], "--seed", "2",
                   "--save-training", "--save-best", *MODEL],
                  on_step=lambda s: seen.append((np.array(s["raw_captions"]).T.flatten().tolist(), list(s["captions"]))))
    assert run.name.startswith("clip_finetuned_on_fiq_")
    val = _rows(run / "validation_metrics.csv")
    assert len(val) == 1 and list(val[0]) == ["epoch", "dress_recall_at10", "dress_recall_at50", "average_recall_at10", "average_recall_at50",
                                              "average_recall"]
    assert float(val[0]["average_recall"]) == (float(val[0]["dress_recall_at10"]) + float(val[0]["dress_recall_at50"])) / 2
    assert list(_rows(run / "train_metrics.csv")[0]) == ["epoch", "loss_itc", "loss_rtc", "loss_align"]
    assert (run / "saved_models" / "tuned_clip_best.pt").exists()          # average_recall > 0 on an 8-image gallery
    # the captions the model was given: the reference's randomiser under random.seed(--seed), then the caption processor
    assert len(seen) == 2 and all(len(flat) == 2 * BATCH and len(caps) == BATCH for flat, caps in seen)
    proc = BlipCaptionProcessor()
    random.seed(2)
    for flat, caps in seen:
        want = [proc(c) for c in generate_randomized_fiq_caption(flat)]
        assert caps == want
        tok = __import__("sprc_amd.tokenizer", fromlist=["BertWordPieceTokenizer"]).BertWordPieceTokenizer()
        kw = dict(padding="max_length", truncation=True, max_length=32, return_tensors="pt")
        assert torch.equal(tok(caps, **kw).input_ids, tok(want, **kw).input_ids)


def test_resume_continues_the_run(world):
    from torch.optim.lr_scheduler import OneCycleLR
    from sprc_amd import blip_fine_tune_2 as ft
    base = ["--dataset", "CIRR", "--validation-frequency", "1", "--model-path", world["ckpt"], "--seed", "9", *MODEL]
    run = ft.main(base + ["--num-epochs", "1"])
    state_file = run / "saved_models" / "training_state.pt"
    first = torch.load(state_file, map_location="cpu", weights_only=False)
    steps_per_epoch = N_TRAIN // BATCH
    assert first["epoch"] == 0 and first["global_step"] == steps_per_epoch and first["drop_step"] == steps_per_epoch and first["dropout_seed"] == 9

    def applied(state):          # optimiser steps that were not skipped: the scaler halves its scale at every skipped one (no growth this early)
        return state["global_step"] - round(math.log2(65536.0 / state["scaler"]["scale"]))

    saved_steps = {float(s["step"]) for s in first["optimizer"]["state"].values()}
    assert saved_steps == {float(applied(first))}
    seen = []

    def hook(s):
        if not seen:
            opt = s["optimizer"]
            st = [opt.state[p] for p in opt.param_groups[0]["params"] if p in opt.state]
            seen.append(dict(lr=opt.param_groups[0]["lr"], beta1=opt.param_groups[0]["betas"][0], global_step=s["global_step"], epoch=s["epoch"],
                             step={float(x["step"]) for x in st}, scale=s["scaler"].get_scale(), growth=s["scaler"]._get_growth_tracker(),
                             drop_step=s["model"]._drop_step, exp_avg=[x["exp_avg"].detach().cpu().clone() for x in st],
                             exp_avg_sq=[x["exp_avg_sq"].detach().cpu().clone() for x in st]))

    again = ft.main(base + ["--num-epochs", "2", "--resume", str(run)], on_step=hook)
    assert again == run
    got = seen[0]
    # the schedule: OneCycleLR's values at the index of the first resumed step, exactly
    p = torch.nn.Parameter(torch.zeros(1))
    ref_opt = torch.optim.AdamW([{"params": [p], "lr": 2e-6, "betas": (0.9, 0.98), "eps": 1e-7, "weight_decay": 0.05}])
    ref_sched = OneCycleLR(ref_opt, max_lr=2e-6, pct_start=1 / 50, steps_per_epoch=steps_per_epoch, epochs=80)
    for _ in range(steps_per_epoch):
        ref_opt.step()
        ref_sched.step()
    assert (got["lr"], got["beta1"]) == (ref_opt.param_groups[0]["lr"], ref_opt.param_groups[0]["betas"][0])
    assert got["epoch"] == 1 and got["global_step"] == steps_per_epoch and got["drop_step"] == steps_per_epoch
    assert got["step"] == saved_steps
    assert got["scale"] == first["scaler"]["scale"] and got["growth"] == first["scaler"]["_growth_tracker"]
    order = sorted(first["optimizer"]["state"])
    assert len(order) == len(got["exp_avg"]) > 300
    assert all(torch.equal(first["optimizer"]["state"][i]["exp_avg"].cpu(), a) and torch.equal(first["optimizer"]["state"][i]["exp_avg_sq"].cpu(), b)
               for i, a, b in zip(order, got["exp_avg"], got["exp_avg_sq"]))
    second = torch.load(state_file, map_location="cpu", weights_only=False)
    assert second["epoch"] == 1 and second["global_step"] == 2 * steps_per_epoch and second["drop_step"] == 2 * steps_per_epoch
    assert {float(s["step"]) for s in second["optimizer"]["state"].values()} == {float(applied(second))}
    assert [r["epoch"] for r in _rows(run / "train_metrics.csv")] == ["0", "1"]
    assert [r["epoch"] for r in _rows(run / "validation_metrics.csv")] == ["0", "1"]
    with pytest.raises(SystemExit, match="batch_size"):
        ft.main(["--dataset", "CIRR", "--num-epochs", "2", "--resume", str(run), "--blip-model-name", "blip2_cir_align_prompt", "--batch-size", "8"])
