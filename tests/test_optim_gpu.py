"""sprc_adamw_step (csrc/optim.hip) and sprc_amd.optim.FusedAdamW: the fused AdamW step of the fine-tuning loops.

The numerical bar is relative, not absolute: torch.optim.AdamW(foreach=False) on the CPU in fp32 (reference A) and in fp64 (reference
B) run the same 12 steps; for each of p / exp_avg / exp_avg_sq the kernel's max |error| against B must be at most 2 x A's own max
|error| against B.  An op-for-op fp32 restatement of the kernel's formula without FMA (numpy) reads 1.00 x / 0.95 x / 1.00 x of torch's
error on these inputs (torch's vectorised CPU code may fuse a multiply-add, nothing else differs); a kernel that reorders the formula or
forms a scalar in fp32 leaves the bar on p within a few steps."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sprc_amd import _lib as L
from sprc_amd.optim import FusedAdamW, chunk_prefix

gpu = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = L.OPT_CHUNK
SIZES = [1, 3, 4, 5, 255, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, 1501]     # the LAST one is placed 4 bytes past a 16-byte boundary
STEPS = 12
EPS, WD, BETA2 = 1e-7, 0.05, 0.98
# what OneCycleLR hands out: lr AND beta1 move every step
LRS = [1e-4 + 8e-5 * k for k in range(STEPS)]
BETA1S = [0.95 - 0.004 * k for k in range(STEPS)]


@functools.lru_cache(maxsize=None)
def _case():
    """(initial parameters, per-step gradients): magnitudes over 1e-7 .. 1e-1, step 5 with exact zeros in every seventh element."""
    g = torch.Generator().manual_seed(1234)
    p0 = [0.05 * torch.randn(n, generator=g) for n in SIZES]
    grads = []
    for k in range(STEPS):
        step = []
        for n in SIZES:
            mag = 10.0 ** (-7.0 + 6.0 * torch.rand(n, generator=g))
            x = mag * torch.sign(torch.randn(n, generator=g))
            if k == 5:
                x[::7] = 0.0
            step.append(x.float())
        grads.append(step)
    return p0, grads


def _hyper(opt, k):
    opt.param_groups[0]["lr"] = LRS[k]
    opt.param_groups[0]["betas"] = (BETA1S[k], BETA2)


def _group(params):
    return [{"params": params, "lr": LRS[0], "betas": (BETA1S[0], BETA2), "eps": EPS, "weight_decay": WD}]


@functools.lru_cache(maxsize=None)
def _torch_reference(dtype):
    """torch.optim.AdamW(foreach=False) on the CPU -> (p, exp_avg, exp_avg_sq) after STEPS steps, one flat fp64 array each."""
    p0, grads = _case()
    params = [torch.nn.Parameter(t.clone().to(dtype)) for t in p0]
    opt = torch.optim.AdamW(_group(params), foreach=False)
    for k in range(STEPS):
        _hyper(opt, k)
        for p, g in zip(params, grads[k]):
            p.grad = g.to(dtype)
        opt.step()
    return tuple(torch.cat([f(p).detach().double().reshape(-1) for p in params]).numpy()
                 for f in (lambda p: p, lambda p: opt.state[p]["exp_avg"], lambda p: opt.state[p]["exp_avg_sq"]))


def _bar(got, what):
    """got: (p, exp_avg, exp_avg_sq) flat arrays.  Prints every figure, then asserts the 2 x bar."""
    a, b = _torch_reference(torch.float32), _torch_reference(torch.float64)
    ratios = []
    for name, x, xa, xb in zip(("p", "exp_avg", "exp_avg_sq"), got, a, b):
        e_k, e_a = float(np.abs(np.asarray(x, dtype=np.float64) - xb).max()), float(np.abs(xa - xb).max())
        print(f"\n[{what}] {name}: max |kernel - fp64| = {e_k:.3e}, max |torch fp32 - fp64| = {e_a:.3e}, ratio {e_k / e_a:.2f}")
        ratios.append((name, e_k, e_a))
    for name, e_k, e_a in ratios:
        assert e_a > 0 and e_k <= 2.0 * e_a, (what, name, e_k, e_a)


def _misaligned(n):
    """n fp32 elements starting 4 bytes past a 16-byte boundary (a view, as a parameter that is a slice of a larger tensor)."""
    base = torch.zeros(n + 8, device=DEV)
    assert base.data_ptr() % 16 == 0
    return base[1:n + 1]


def _device_tensors(p0):
    out = []
    for i, t in enumerate(p0):
        if i == len(p0) - 1:
            views = [_misaligned(t.numel()) for _ in range(4)]
        else:
            views = [torch.zeros(t.numel(), device=DEV) for _ in range(4)]
        views[0].copy_(t)
        out.append(views)                              # [p, g, m, v]
    return out


class _Call:
    """sprc_adamw_step through the ctypes binding: table and prefix built and uploaded here."""

    def __init__(self, tensors):
        self.tensors = tensors
        rows = np.array([[p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()] for p, g, m, v in tensors], dtype=np.int64)
        self.first = chunk_prefix(rows[:, 4])
        self.table = torch.from_numpy(rows.reshape(-1)).to(DEV)
        self.prefix = torch.from_numpy(self.first).to(DEV)
        self.step = torch.zeros((), device=DEV)
        self.scratch = torch.zeros(16, device=DEV)

    def __call__(self, lr, beta1, grad_scale=None, found_inf=None, wd=WD):
        a = L.AdamWArgs()
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = lr, beta1, BETA2, EPS, wd
        a.grad_scale = grad_scale.data_ptr() if grad_scale is not None else None
        a.found_inf = found_inf.data_ptr() if found_inf is not None else None
        a.step, a.scratch = self.step.data_ptr(), self.scratch.data_ptr()
        L.check(L.load().sprc_adamw_step(self.table.data_ptr(), len(self.tensors), self.prefix.data_ptr(), int(self.first[-1]), C.byref(a),
                                         torch.cuda.current_stream().cuda_stream), "sprc_adamw_step")

    def flat(self):
        torch.cuda.synchronize()
        return tuple(torch.cat([t[i].reshape(-1) for t in self.tensors]).cpu().numpy() for i in (0, 2, 3))


def _run_lib(steps=range(STEPS), scale=None, skip_before=()):
    p0, grads = _case()
    call = _Call(_device_tensors(p0))
    gs = torch.tensor([scale], device=DEV) if scale is not None else None
    for k in steps:
        for (p, g, m, v), x in zip(call.tensors, grads[k]):
            g.copy_(x * scale if scale is not None else x)
        if k in skip_before:                           # a call that found_inf skips, made just before step k's real call
            before = [t.clone() for views in call.tensors for t in views] + [call.step.clone()]
            call(LRS[k], BETA1S[k], grad_scale=gs, found_inf=torch.ones(1, device=DEV))
            torch.cuda.synchronize()
            after = [t for views in call.tensors for t in views] + [call.step]
            assert all(torch.equal(x, y) for x, y in zip(before, after))          # p, g, m, v and step: bit for bit
        call(LRS[k], BETA1S[k], grad_scale=gs, found_inf=torch.zeros(1, device=DEV) if skip_before else None)
    return call


@gpu
def test_kernel_against_torch_calibrated_by_fp64():
    call = _run_lib()
    assert float(call.step) == STEPS
    _bar(call.flat(), "sprc_adamw_step")
    # the optimiser class drives the same kernel: same bits, the misaligned parameter included
    p0, grads = _case()
    params = [torch.nn.Parameter(views[0]) for views in _device_tensors(p0)]
    assert params[-1].data_ptr() % 16 == 4
    opt = FusedAdamW(_group(params))
    for k in range(STEPS):
        _hyper(opt, k)
        for p, g in zip(params, grads[k]):
            p.grad = g.to(DEV)
        opt.step()
    torch.cuda.synchronize()
    got = tuple(torch.cat([f(p).detach().reshape(-1) for p in params]).cpu().numpy()
                for f in (lambda p: p, lambda p: opt.state[p]["exp_avg"], lambda p: opt.state[p]["exp_avg_sq"]))
    assert all(np.array_equal(x, y) for x, y in zip(got, call.flat()))
    assert float(opt.state[params[0]]["step"]) == STEPS


@gpu
def test_skip_and_scale_are_bit_exact():
    plain = _run_lib(range(4)).flat()
    skipped = _run_lib(range(4), skip_before=(0, 2))
    assert float(skipped.step) == 4                                    # the skipped calls did not count
    assert all(np.array_equal(x, y) for x, y in zip(plain, skipped.flat()))
    p0, grads = _case()
    scaled = _run_lib(range(4), scale=65536.0)
    assert all(np.array_equal(x, y) for x, y in zip(plain, scaled.flat()))
    for (p, g, m, v), x in zip(scaled.tensors, grads[3]):              # g is read, never written
        assert torch.equal(g.cpu(), x * 65536.0) and bool(torch.isfinite(g).all())


@gpu
def test_table_of_400_tensors_equals_400_single_calls():
    rng = np.random.default_rng(7)
    sizes = [int(n) for n in rng.integers(1, 3 * CHUNK + 1, size=400)]
    g = torch.Generator().manual_seed(5)
    init = [[0.05 * torch.randn(n, generator=g), 1e-3 * torch.randn(n, generator=g), 1e-3 * torch.randn(n, generator=g),
             1e-6 * torch.rand(n, generator=g)] for n in sizes]
    one = _Call([[t.to(DEV) for t in views] for views in init])
    one.step.fill_(6)
    one(3e-4, 0.93)
    singles = []
    for views in init:
        c = _Call([[t.to(DEV) for t in views]])
        c.step.fill_(6)
        c(3e-4, 0.93)
        singles.append(c)
    torch.cuda.synchronize()
    assert float(one.step) == 7
    for views, c in zip(one.tensors, singles):
        for x, y in zip(views, c.tensors[0]):
            assert torch.equal(x, y)
    assert not torch.equal(one.tensors[0][0].cpu(), init[0][0])


@gpu
def test_optimizer_class():
    p0, grads = _case()

    def fresh():
        return [torch.nn.Parameter(t.clone().to(DEV)) for t in p0]

    def steps(opt, params, ks):
        for k in ks:
            _hyper(opt, k)
            for p, g in zip(params, grads[k]):
                if p.requires_grad and p is not params[2]:
                    p.grad = g.to(DEV)
            opt.step()

    # parameters without a gradient are untouched and get no state
    params = fresh()
    opt = FusedAdamW(_group(params))
    steps(opt, params, range(2))
    assert torch.equal(params[2].detach().cpu(), p0[2]) and params[2] not in opt.state and len(opt.state) == len(params) - 1
    assert not torch.equal(params[3].detach().cpu(), p0[3])
    # weight_decay = 0
    params = fresh()
    opt = FusedAdamW([{**_group(params)[0], "weight_decay": 0.0}])
    ref = [torch.nn.Parameter(t.clone()) for t in p0]
    ropt = torch.optim.AdamW([{**_group(ref)[0], "weight_decay": 0.0}], foreach=False)
    for p, q, g in zip(params, ref, grads[0]):
        p.grad, q.grad = g.to(DEV), g.clone()
    opt.step()
    ropt.step()
    for p, q in zip(params, ref):
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=1e-6, atol=1e-9)
    with pytest.raises(ValueError, match="amsgrad"):
        FusedAdamW(_group(fresh()), amsgrad=True)
    with pytest.raises(ValueError, match="fp32 CUDA"):
        FusedAdamW(_group([torch.nn.Parameter(torch.zeros(3))]))

    # FusedAdamW -> torch.optim.AdamW -> FusedAdamW through state dicts: 4 steps under each, inside the bar of the first test
    def every(opt, params, ks):
        for k in ks:
            _hyper(opt, k)
            for p, g in zip(params, grads[k]):
                p.grad = g.to(DEV)
            opt.step()

    params = fresh()
    a = FusedAdamW(_group(params))
    every(a, params, range(0, 4))
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 4 and sd["state"][0]["step"].device.type == "cpu"
    b = torch.optim.AdamW(_group(params))
    b.load_state_dict(sd)
    every(b, params, range(4, 8))
    c = FusedAdamW(_group(params))
    c.load_state_dict(b.state_dict())
    assert float(c.state[params[0]]["step"]) == 8
    every(c, params, range(8, 12))
    torch.cuda.synchronize()
    _bar(tuple(torch.cat([f(p).detach().reshape(-1) for p in params]).cpu().numpy()
               for f in (lambda p: p, lambda p: c.state[p]["exp_avg"], lambda p: c.state[p]["exp_avg_sq"])), "FusedAdamW -> AdamW -> FusedAdamW")
    # a state whose parameters disagree on `step` is refused
    bad = b.state_dict()
    bad["state"][1] = dict(bad["state"][1], step=torch.tensor(3.0))
    with pytest.raises(ValueError, match="disagree on `step`"):
        FusedAdamW(_group(params)).load_state_dict(bad)
    kept = {p: (c.state[p]["exp_avg"].clone(), float(c.state[p]["step"])) for p in params}
    with pytest.raises(ValueError, match="disagree on `step`"):
        c.load_state_dict(bad)                     # refused before anything is changed
    assert all(p in c.state and torch.equal(c.state[p]["exp_avg"], kept[p][0]) and float(c.state[p]["step"]) == kept[p][1] == 12 for p in params)


def test_argument_validation_needs_no_launch():
    """Refused before any launch (the pointers below are never dereferenced): runs without a GPU."""
    lib = L.load()
    a = L.AdamWArgs()
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = 1e-4, 0.9, 0.98, 1e-7, 0.05
    a.step, a.scratch = 0x1000, 0x2000
    ok = (0x3000, 1, 0x4000, 1)
    assert lib.sprc_adamw_step(None, 1, 0x4000, 1, C.byref(a), None) == -1 and b"null" in lib.sprc_last_error()
    assert lib.sprc_adamw_step(0x3000, 1, None, 1, C.byref(a), None) == -1 and b"null" in lib.sprc_last_error()
    assert lib.sprc_adamw_step(0x3000, 0, 0x4000, 0, C.byref(a), None) == -1 and b"n_tensors" in lib.sprc_last_error()
    # every tensor has at least one chunk: a prefix over 3 tensors cannot end at 2
    assert lib.sprc_adamw_step(0x3000, 3, 0x4000, 2, C.byref(a), None) == -1 and b"disagrees with the prefix" in lib.sprc_last_error()
    for field, value, word in (("step", None, b"null"), ("scratch", None, b"null"), ("beta1", 1.0, b"betas"), ("beta2", -0.1, b"betas"),
                               ("eps", 0.0, b"eps")):
        keep = getattr(a, field)
        setattr(a, field, value)
        assert lib.sprc_adamw_step(*ok, C.byref(a), None) == -1 and word in lib.sprc_last_error(), field
        setattr(a, field, keep)
    with pytest.raises(L.SprcError, match="sprc_adamw_step"):
        L.check(lib.sprc_adamw_step(None, 1, None, 1, None, None), "sprc_adamw_step")
    assert list(chunk_prefix([1, CHUNK, CHUNK + 1])) == [0, 1, 2, 4]
    with pytest.raises(ValueError):
        chunk_prefix([4, 0])


# ---- in the reference's loop on the model ---------------------------------------------------------------------------------------
class _Tok:
    def __init__(self, ids, mask):
        self.ids, self.mask = ids, mask

    def __call__(self, text, **kw):
        from sprc_amd.tokenizer import TokenBatch
        return TokenBatch(self.ids, self.mask)


def _train_case(golden_dir):
    """The case of test_train_gpu's reference-loop test, rebuilt from tests/golden/train_eva.npz: eval-mode model (no dropout)."""
    from sprc_amd import synth
    from sprc_amd.config import get_config
    from sprc_amd.model import Blip2QformerCirAlignPrompt
    g = np.load(golden_dir / "train_eva.npz", allow_pickle=False)
    cfg = get_config(str(g["model_type"]), vit_depth=int(g["vit_depth"]))
    sd = synth.make_state_dict(cfg, seed=int(g["seed"]))
    B = int(g["batch"])
    model = Blip2QformerCirAlignPrompt(cfg=cfg, compute_dtype="fp32", max_batch=8)
    assert not model.load_state_dict(sd, strict=False).missing_keys
    model = model.to(DEV).eval()
    model.tokenizer = _Tok(torch.from_numpy(g["input_ids"]), torch.from_numpy(g["attention_mask"]))
    images = synth.make_images(2 * B, seed=int(g["seed"]))
    return g, model, {"image": images[:B].to(DEV), "target": images[B:].to(DEV), "text_input": ["caption"] * B}


@gpu
def test_fused_adamw_behind_the_stock_grad_scaler_in_the_reference_loop(golden_dir):
    g, model, batch = _train_case(golden_dir)
    opt = FusedAdamW([{"params": [p for p in model.parameters() if p.requires_grad], "lr": 2e-5, "betas": (0.9, 0.98), "eps": 1e-7,
                       "weight_decay": 0.05}])

    def one_step(scaler):
        opt.zero_grad()
        with torch.cuda.amp.autocast():
            d = model(batch)
            loss = d["loss_itc"] + 0.4 * d["loss_rtc"] + 0.4 * d["loss_align"]
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
        return float(loss)

    scaler = torch.cuda.amp.GradScaler()
    trunk0 = model.state_dict()["visual_encoder.blocks.0.attn.qkv.weight"].clone()
    hist = [one_step(scaler) for _ in range(4)]
    print(f"\n[train loop, FusedAdamW] loss over 4 steps: {[round(x, 4) for x in hist]}")
    assert hist[-1] < hist[0] - 1e-3
    assert torch.equal(model.state_dict()["visual_encoder.blocks.0.attn.qkv.weight"], trunk0)
    with torch.no_grad():
        after = model(batch)
    assert float(after["loss_itc"]) < float(g["loss_itc"])                      # the inference engine was rebuilt from the moved weights
    stepped = [p for p in model.parameters() if p in opt.state]
    assert len(stepped) > 300 and float(opt.state[stepped[0]]["step"]) == 4
    assert not any(n.startswith(("itm_head.", "Qformer.cls.")) for n, p in model.named_parameters() if p in opt.state)
    assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")

    # scaled gradients overflow to inf: the step is skipped on the device, the scaler halves its scale.  The overflow is the one the
    # reference's loop has: 16-bit operands under autocast -- at 2^120 the fp16 operand copies of the backward are inf.  (The exact-fp32
    # products of the four steps above hold 2^120 x these gradients: fp32 reaches 2^128, nothing overflows and the step is APPLIED.)
    model.train_products = "fp16"
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    state0 = {n: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for n, p in model.named_parameters() if p in opt.state}
    big = torch.cuda.amp.GradScaler(init_scale=2.0 ** 120)
    one_step(big)
    torch.cuda.synchronize()
    grads = [p.grad for p in stepped]
    print(f"[overflow step] {sum(int(not torch.isfinite(x).all()) for x in grads)} of {len(grads)} gradients are not finite")
    assert any(not torch.isfinite(x).all() for x in grads)                     # the skip has the cause it claims
    assert all(torch.equal(p.detach(), before[n]) for n, p in model.named_parameters())
    assert all(torch.equal(opt.state[p]["exp_avg"], state0[n][0]) and torch.equal(opt.state[p]["exp_avg_sq"], state0[n][1])
               for n, p in model.named_parameters() if p in opt.state)
    assert float(opt.state[stepped[0]]["step"]) == 4 and float(next(iter(opt.state_dict()["state"].values()))["step"]) == 4
    assert big.get_scale() == 2.0 ** 119
