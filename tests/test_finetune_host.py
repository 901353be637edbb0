"""Host side of the fine-tuning entry point (sprc_amd/blip_fine_tune_2.py), no GPU: the FashionIQ caption randomiser against what
the reference's function returned (tests/golden/fiq_randomized_captions.json, tools/gen_finetune_golden.py), the two learning-rate
schedules against OneCycleLR built with the reference's literal arguments (blip_fine_tune_2.py:260, :95), the argument defaults
against the reference's (:370-391), the refusal of a CIRR run longer than its schedule, and the appending CSV writer."""
import csv
import json
import random

import pytest
import torch
from torch.optim.lr_scheduler import OneCycleLR


def test_caption_randomiser_matches_the_reference(golden_dir):
    from sprc_amd.processors import generate_randomized_fiq_caption
    g = json.loads((golden_dir / "fiq_randomized_captions.json").read_text())
    flat = g["flattened_captions"]
    assert len(flat) == 128 and any(c[-1] in ".?, " for c in flat) and any(c[0] in ".?, " for c in flat)
    forms = set()
    for seed in range(4):
        random.seed(seed)
        got = generate_randomized_fiq_caption(list(flat))
        assert got == g["by_seed"][str(seed)], seed
        forms |= {(" and " in c) for c in got}
    assert forms == {True, False}                 # joined and single forms both occur
    # the strict comparisons: a draw of exactly 0.25 / 0.5 / 0.75 takes the LAST branch (caption 2 alone), as in the reference
    real = random.random
    try:
        for edge, want in ((0.25, "Two"), (0.5, "Two"), (0.75, "Two"), (0.2499, "One and two"), (0.2501, "Two and one"), (0.5001, "One"),
                           (0.7501, "Two")):
            random.random = lambda e=edge: e
            assert generate_randomized_fiq_caption(["one.", " two?"]) == [want], edge
    finally:
        random.random = real


def _sequence(opt, sched, n):
    out = []
    for _ in range(n):
        out.append((opt.param_groups[0]["lr"], opt.param_groups[0]["betas"][0]))
        opt.step()
        sched.step()
    return out


def _adamw(lr):
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.zeros(3)
    return torch.optim.AdamW([{"params": [p], "lr": lr, "betas": (0.9, 0.98), "eps": 1e-7, "weight_decay": 0.05}])


def test_schedules_are_the_references():
    from sprc_amd import blip_fine_tune_2 as ft
    lr, spe = 2e-6, 7
    # CIRR (:260): 80 epochs whatever --num-epochs says
    a, b = _adamw(lr), _adamw(lr)
    got = _sequence(a, ft.build_scheduler(a, "cirr", lr, spe, num_epochs=50), 200)
    want = _sequence(b, OneCycleLR(b, max_lr=lr, pct_start=1 / 50, steps_per_epoch=spe, epochs=80), 200)
    assert got == want and len({x for x, _ in got}) > 100 and len({m for _, m in got}) > 100      # lr AND beta1 move every step
    # FashionIQ (:95)
    num_epochs = 30
    a, b = _adamw(lr), _adamw(lr)
    got = _sequence(a, ft.build_scheduler(a, "fashioniq", lr, spe, num_epochs=num_epochs), 200)
    want = _sequence(b, OneCycleLR(b, max_lr=lr, pct_start=1.5 / num_epochs, div_factor=100., steps_per_epoch=spe, epochs=num_epochs), 200)
    assert got == want and got[0][0] == pytest.approx(lr / 100.)
    assert ft.ADAMW == {"betas": (0.9, 0.98), "eps": 1e-7, "weight_decay": 0.05}


def test_argument_defaults_are_the_references(golden_dir):
    from sprc_amd import blip_fine_tune_2 as ft
    want = json.loads((golden_dir / "finetune_arg_defaults.json").read_text())
    assert len(want) == 17
    parser = ft.build_parser()
    actions = {s: act for act in parser._actions for s in act.option_strings}
    for flag, spec in want.items():
        assert flag in actions, flag
        assert actions[flag].default == spec["default"] and type(actions[flag].default) is type(spec["default"]), flag
        assert bool(actions[flag].required) == spec["required"], flag
    a = parser.parse_args(["--dataset", "CIRR"])
    assert (a.train_products, a.optimizer, a.dtype, a.max_steps, a.seed, a.resume, a.model_path) == ("fp16", "fused", "fp16", None, None, None, None)
    assert set(ft.hyper_params(a)) == {"num_epochs", "num_workers", "blip_model_name", "backbone", "learning_rate", "batch_size",
                                       "validation_frequency", "transform", "target_ratio", "save_training", "save_best", "data_path",
                                       "loss_rtc", "loss_align", "loss_itm", "save_memory"}


def test_cirr_run_longer_than_its_schedule_is_refused_before_anything_is_built(monkeypatch):
    from sprc_amd import blip_fine_tune_2 as ft
    import sprc_amd.model as M

    def boom(*a, **k):
        raise AssertionError("a model was built")

    monkeypatch.setattr(M, "load_model_and_preprocess", boom)
    with pytest.raises(SystemExit, match="80"):
        ft.main(["--dataset", "CIRR", "--num-epochs", "81", "--blip-model-name", "blip2_cir_align_prompt", "--model-path", "nowhere.pt"])
    assert ft.check_args(ft.build_parser().parse_args(["--dataset", "cirr", "--num-epochs", "80"])) == "cirr"
    assert ft.check_args(ft.build_parser().parse_args(["--dataset", "fashionIQ", "--num-epochs", "300"])) == "fashioniq"
    with pytest.raises(SystemExit, match="at least 2 epochs"):       # pct_start = 1.5 / num_epochs > 1: torch's OneCycleLR refuses it
        ft.main(["--dataset", "fashionIQ", "--num-epochs", "1", "--blip-model-name", "blip2_cir_align_prompt", "--model-path", "nowhere.pt"])
    with pytest.raises(ValueError):
        ft.main(["--dataset", "imagenet"])
    with pytest.raises(SystemExit, match="targetpad"):
        ft.main(["--dataset", "CIRR", "--num-epochs", "2", "--transform", "squarepad"])


def test_csv_writer_appends(tmp_path):
    from sprc_amd.blip_fine_tune_2 import append_csv_row
    p = tmp_path / "train_metrics.csv"
    append_csv_row(p, {"epoch": 0, "loss_itc": 1.5, "loss_rtc": 0.25, "loss_align": 0.125})
    append_csv_row(p, {"epoch": 1, "loss_itc": 1.25, "loss_rtc": 0.5, "loss_align": 0.0625})
    rows = list(csv.reader(open(p, newline="")))
    assert rows == [["epoch", "loss_itc", "loss_rtc", "loss_align"], ["0", "1.5", "0.25", "0.125"], ["1", "1.25", "0.5", "0.0625"]]
    with pytest.raises(ValueError, match="columns"):
        append_csv_row(p, {"epoch": 2, "loss_itc": 1.0})
    q = tmp_path / "validation_metrics.csv"
    append_csv_row(q, {"epoch": 0, "mean(R@5+R_s@1)": 50.0})
    assert open(q).read().splitlines() == ["epoch,mean(R@5+R_s@1)", "0,50.0"]
