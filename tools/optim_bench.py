#!/usr/bin/env python3
"""The optimiser step of the fine-tuning loop, measured: sprc_amd.optim.FusedAdamW against torch.optim.AdamW (its default foreach
path) and torch.optim.AdamW(fused=True), each behind the stock GradScaler.

(a) the step alone on the real shape set (the 337 trainable tensors of the ViT-g model that receive gradients, 186.1 M elements):
    `scaler.step(opt); scaler.update()` between HIP events, the three optimisers alternating in one process, warm-up excluded,
    median / min / max over the timed steps.  Traffic floor: 28 bytes per element (read p, g, m, v; write p, m, v).
(b) the whole training step (batch 32, fp16 products, fp16 frozen trunk) with each optimiser, same method.

    python tools/optim_bench.py [steps=24] [train_steps=8] [out=profiles/finetune_optim.txt]
"""
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sprc_amd import synth  # noqa: E402
from sprc_amd.config import get_config  # noqa: E402
from sprc_amd.optim import FusedAdamW  # noqa: E402
from sprc_amd.train import TrainStep  # noqa: E402

DEV = "cuda:0"
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 24
TRAIN_STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 8
OUT = Path(sys.argv[3]) if len(sys.argv) > 3 else ROOT / "profiles" / "finetune_optim.txt"
WARMUP = 3
GROUP = dict(lr=2e-6, betas=(0.9, 0.98), eps=1e-7, weight_decay=0.05)
KINDS = {"FusedAdamW": lambda ps: FusedAdamW([{"params": ps, **GROUP}]),
         "torch AdamW (foreach)": lambda ps: torch.optim.AdamW([{"params": ps, **GROUP}]),
         "torch AdamW (fused=True)": lambda ps: torch.optim.AdamW([{"params": ps, **GROUP}], fused=True)}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(ms):
    return f"median {statistics.median(ms):7.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f}, n = {len(ms)})"


def optimiser_step():
    cfg = get_config("pretrain")
    shapes = [tuple(shape) for name, shape, _ in synth.param_specs(cfg) if not name.startswith("visual_encoder.") and TrainStep._trains(name)]
    shapes.append(())                                                  # temp
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    g = torch.Generator(device=DEV).manual_seed(0)
    master = [1e-3 * torch.randn(s, device=DEV, generator=g) * 65536.0 for s in shapes]       # scaled gradients, as backward leaves them
    runs = {}
    for kind, make in KINDS.items():
        ps = [torch.nn.Parameter(0.02 * torch.randn(s, device=DEV, generator=g)) for s in shapes]
        for p in ps:
            p.grad = torch.empty_like(p)
        runs[kind] = dict(params=ps, opt=make(ps), scaler=torch.amp.GradScaler("cuda"), ms=[])
    for r in runs.values():
        r["scaler"].scale(torch.zeros((), device=DEV))                 # creates the scale tensor, as the loop's scaler.scale(loss) does

    def one(r):
        r["scaler"].step(r["opt"])
        r["scaler"].update()

    for i in range(WARMUP + STEPS):
        for r in runs.values():
            torch._foreach_copy_([p.grad for p in r["params"]], master)       # unscale_ works in place: fresh scaled gradients every step
            ms = timed(lambda: one(r))
            if i >= WARMUP:
                r["ms"].append(ms)
    say(f"(a) optimiser step behind GradScaler: {len(shapes)} tensors, {n} elements ({n * 28 / 1e9:.2f} GB of traffic at 28 B / element)")
    for kind, r in runs.items():
        med = statistics.median(r["ms"])
        say(f"    {kind:26s} {summary(r['ms'])}  = {n * 28 / med / 1e9:.2f} TB/s of the 28-B traffic")
    return runs


def training_step():
    from sprc_amd.model import Blip2QformerCirAlignPrompt
    from sprc_amd.tokenizer import TokenBatch
    B = 32
    cfg = get_config("pretrain")
    ids, mask, _ = synth.make_queries(B, B, seed=1)
    images = synth.make_images(2 * B, seed=0)
    model = Blip2QformerCirAlignPrompt(cfg=cfg, compute_dtype="fp32", max_batch=B, train_vit_dtype="fp16", train_products="fp16")
    model.load_state_dict(synth.make_state_dict(cfg, seed=0), strict=False)
    model = model.to(DEV)
    model.tokenizer = lambda text, **kw: TokenBatch(ids[:len(text)], mask[:len(text)])
    batch = {"image": images[:B].to(DEV), "target": images[B:].to(DEV), "text_input": ["caption"] * B}
    ps = [p for p in model.parameters() if p.requires_grad]
    runs = {kind: dict(opt=make(ps), scaler=torch.amp.GradScaler("cuda"), ms=[]) for kind, make in KINDS.items()}

    def one(r):
        r["opt"].zero_grad()
        with torch.amp.autocast("cuda"):
            d = model(batch)
            loss = d["loss_itc"] + 0.4 * d["loss_rtc"] + 0.4 * d["loss_align"]
        r["scaler"].scale(loss).backward()
        r["scaler"].step(r["opt"])
        r["scaler"].update()

    for i in range(WARMUP + TRAIN_STEPS):
        for r in runs.values():
            ms = timed(lambda: one(r))
            if i >= WARMUP:
                r["ms"].append(ms)
    say(f"(b) whole training step, batch {B}, fp16 products, fp16 frozen ViT-g trunk, forward + backward + optimiser step")
    for kind, r in runs.items():
        say(f"    {kind:26s} {summary(r['ms'])}")


if __name__ == "__main__":
    say(f"# tools/optim_bench.py on {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    optimiser_step()
    torch.cuda.empty_cache()
    if TRAIN_STEPS > 0:
        training_step()
    OUT.parent.mkdir(parents=True, exist_ok=True)
    OUT.write_text("\n".join(lines) + "\n")
