"""FusedAdamW: `torch.optim.AdamW` with the update in one HIP launch per parameter group (sprc_adamw_step, csrc/optim.hip).

The reference's loops (blip_fine_tune_2.py:257-259, :90-93) build `optim.AdamW([{params, lr, betas, eps, weight_decay}])` and step it through
`GradScaler` (:302).  This class takes the same param-group keys, reads `lr` / `betas` from `param_groups` at every step (OneCycleLR
rewrites both), works behind the stock `torch.cuda.amp.GradScaler` -- the scale and the inf flag reach the kernel as device pointers,
`step()` never reads either on the host -- and saves / loads the state-dict layout of `torch.optim.AdamW`, so a run can move between
the two classes.  The arithmetic is torch's single-tensor AdamW, operation for operation (include/sprc.h "Optimiser step").

What stays torch's behind GradScaler: the inf CHECK.  `GradScaler.step` still makes one foreach pass over the gradients
(`_amp_foreach_non_finite_check_and_unscale_` with a scale of 1) to produce `found_inf` -- about 8 bytes per element next to the 28 the
kernel moves; the unscale itself, the skip and the update are the kernel's.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import numpy as np
import torch

from . import _lib as L

_TENSOR_WORDS = C.sizeof(L.OptTensor) // 8            # an sprc_opt_tensor as int64 words: p, g, m, v, n
assert C.sizeof(L.OptTensor) == 40


def chunk_prefix(sizes) -> np.ndarray:
    """int32 [len(sizes) + 1]: prefix sums of ceil(n / SPRC_OPT_CHUNK), the `chunk_first` table of sprc_adamw_step."""
    sizes = np.asarray(list(sizes), dtype=np.int64)
    if sizes.size == 0 or (sizes < 1).any():
        raise ValueError("chunk_prefix: at least one tensor, every tensor with n >= 1")
    first = np.zeros(sizes.size + 1, dtype=np.int64)
    np.cumsum((sizes + L.OPT_CHUNK - 1) // L.OPT_CHUNK, out=first[1:])
    if first[-1] >= 2 ** 31:
        raise ValueError("chunk_prefix: too many elements for one call")
    return first.astype(np.int32)


class _Table:
    """The pointer table of one group on the device.  Every step writes it into a FRESH pinned host tensor and copies that on the
    current stream: torch's caching host allocator hands a pinned block out again only after the copies that read it have finished,
    so nothing here waits for the GPU and no buffer is rewritten under a copy in flight."""

    def __init__(self, device):
        self.device, self.dev = device, None

    def upload(self, rows: np.ndarray, first: np.ndarray):
        n = rows.shape[0]
        need = n * 40 + (n + 1) * 4
        if self.dev is None or need > self.dev.numel():
            self.dev = torch.empty(max(2 * need, 4096), dtype=torch.uint8, device=self.device)
        h = torch.empty(need, dtype=torch.uint8, pin_memory=True)
        buf = h.numpy()
        buf[:n * 40].view(np.int64).reshape(n, _TENSOR_WORDS)[:] = rows
        buf[n * 40:].view(np.int32)[:] = first
        self.dev[:need].copy_(h, non_blocking=True)
        return self.dev.data_ptr(), self.dev.data_ptr() + n * 40


class FusedAdamW(torch.optim.Optimizer):
    """AdamW (decoupled weight decay) over fp32 CUDA parameters, one sprc_adamw_step call per parameter group.

    One difference from torch.optim.AdamW: the applied-step count `t` of the bias corrections is kept per GROUP, on the device, not
    per parameter.  A parameter that first receives a gradient at the group's step k > 1 (or is loaded without state next to
    parameters with state) is corrected for t = k where torch would start it at t = 1.  In the model's loops every trained tensor
    receives its gradient from the first step on, where the two agree."""

    _step_supports_amp_scaling = True        # GradScaler.step then registers `grad_scale` / `found_inf` on this object and calls step()

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False):
        # the keys torch.optim.AdamW keeps in a param group, so that a state dict saved here loads there (its load_state_dict
        # takes the SAVED groups whole)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._gstate: Dict[int, dict] = {}
        for g in self.param_groups:
            self._check_group(g)
            self._check_params(g)

    @staticmethod
    def _check_group(g):
        if g.get("amsgrad") or g.get("maximize"):
            raise ValueError("FusedAdamW: amsgrad and maximize are not implemented (the reference's loops use neither)")
        if not 0.0 <= float(g["lr"]):
            raise ValueError(f"FusedAdamW: lr {g['lr']}")
        if not (0.0 <= g["betas"][0] < 1.0 and 0.0 <= g["betas"][1] < 1.0):
            raise ValueError(f"FusedAdamW: betas {g['betas']}")
        if not g["eps"] > 0.0:
            raise ValueError(f"FusedAdamW: eps {g['eps']} (the kernel divides by sqrt(v) / bc + eps: eps must be > 0)")
        if not 0.0 <= g["weight_decay"]:
            raise ValueError(f"FusedAdamW: weight_decay {g['weight_decay']}")

    @staticmethod
    def _check_params(g):
        devs = set()
        for p in g["params"]:
            if p.dtype != torch.float32 or not p.is_cuda:
                raise ValueError(f"FusedAdamW: parameters must be fp32 CUDA tensors (got {p.dtype} on {p.device}); the update is a "
                                 "HIP kernel, there is no CPU path")
            if not p.is_contiguous():
                raise ValueError("FusedAdamW: parameters must be contiguous")
            devs.add(p.device)
        if len(devs) > 1:
            raise ValueError(f"FusedAdamW: the parameters of one group must live on one device (got {sorted(map(str, devs))})")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_gstate"):
            self._check_group(self.param_groups[-1])
            self._check_params(self.param_groups[-1])

    # ---- per-group device state -----------------------------------------------------------------------------------------------
    def _group_state(self, gi: int, device) -> dict:
        gs = self._gstate.get(gi)
        if gs is None:
            gs = self._gstate[gi] = dict(step=torch.zeros((), dtype=torch.float32, device=device),
                                         scratch=torch.zeros(16, dtype=torch.float32, device=device), table=_Table(device), flat=[])
        return gs

    def _new_state(self, gs: dict, params, exp_avg=None, exp_avg_sq=None):
        """exp_avg / exp_avg_sq of `params` as views into ONE flat buffer each (zeros, or copies of the given tensors)."""
        pad = lambda n: (n + 63) // 64 * 64              # every view starts on a 256-byte boundary: the kernel's 16-byte accesses
        total = sum(pad(p.numel()) for p in params)
        dev = params[0].device
        m, v = torch.zeros(total, dtype=torch.float32, device=dev), torch.zeros(total, dtype=torch.float32, device=dev)
        gs["flat"].append((m, v))
        o = 0
        for i, p in enumerate(params):
            n = p.numel()
            st = self.state[p]
            st["step"] = gs["step"]                      # the group's counter: one applied-step count for every tensor of the group
            st["exp_avg"], st["exp_avg_sq"] = m[o:o + n].view_as(p), v[o:o + n].view_as(p)
            if exp_avg is not None:
                st["exp_avg"].copy_(exp_avg[i])
                st["exp_avg_sq"].copy_(exp_avg_sq[i])
            o += pad(n)

    # ---- the step -------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        lib = L.load()
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            live = [p for p in group["params"] if p.grad is not None and p.numel() > 0]      # grad None: skipped, as torch does
            if not live:
                continue
            dev = live[0].device
            gs = self._group_state(gi, dev)
            fresh = [p for p in live if "exp_avg" not in self.state[p]]
            if fresh:
                self._new_state(gs, fresh)
            rows = np.empty((len(live), _TENSOR_WORDS), dtype=np.int64)
            for i, p in enumerate(live):
                g = p.grad
                if g.is_sparse or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous() or g.numel() != p.numel():
                    raise ValueError("FusedAdamW: gradients must be dense contiguous fp32 tensors on the parameter's device")
                st = self.state[p]
                rows[i] = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
            first = chunk_prefix(rows[:, 4])
            with torch.cuda.device(dev):
                t_ptr, c_ptr = gs["table"].upload(rows, first)
                a = L.AdamWArgs()
                a.lr, a.beta1, a.beta2 = float(group["lr"]), float(group["betas"][0]), float(group["betas"][1])
                a.eps, a.weight_decay = float(group["eps"]), float(group["weight_decay"])
                for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
                    if t is not None:
                        if t.dtype != torch.float32 or t.device != dev or t.numel() != 1:
                            raise ValueError(f"FusedAdamW: {name} must be one fp32 element on {dev} (got {t.dtype}, {t.device}, {t.numel()})")
                        setattr(a, name, t.data_ptr())
                a.step, a.scratch = gs["step"].data_ptr(), gs["scratch"].data_ptr()
                L.check(lib.sprc_adamw_step(t_ptr, len(live), c_ptr, int(first[-1]), C.byref(a), torch.cuda.current_stream(dev).cuda_stream),
                        "sprc_adamw_step")
        return loss

    # ---- checkpoints: the layout of torch.optim.AdamW -----------------------------------------------------------------------------
    def state_dict(self):
        """As torch.optim.AdamW's: per parameter `step` (a CPU fp32 scalar, a COPY of the group's counter), `exp_avg`, `exp_avg_sq`."""
        sd = super().state_dict()
        steps = {}
        state = {}
        for k, st in sd["state"].items():
            key = st["step"].data_ptr()
            if key not in steps:
                steps[key] = st["step"].detach().cpu()
            state[k] = {"step": steps[key].clone(), "exp_avg": st["exp_avg"], "exp_avg_sq": st["exp_avg_sq"]}
        sd["state"] = state
        return sd

    def load_state_dict(self, state_dict):
        """Accepts a state dict of this class or of torch.optim.AdamW.  One applied-step count per group: a state whose parameters
        disagree on `step` is refused.  Everything is checked before anything is changed: a refused state dict leaves the optimiser as
        it was.  The load-state-dict hooks of torch.optim.Optimizer run as in the base class."""
        state_dict = state_dict.copy()
        for pre_hook in self._optimizer_load_state_dict_pre_hooks.values():
            hook_result = pre_hook(self, state_dict)
            if hook_result is not None:
                state_dict = hook_result
        groups, saved = self.param_groups, state_dict["param_groups"]
        if len(groups) != len(saved) or any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved)):
            raise ValueError("FusedAdamW.load_state_dict: the parameter groups do not match the optimiser's (count or sizes)")
        plan = []
        for gi, (g, s) in enumerate(zip(groups, saved)):
            hyper = {k: v for k, v in s.items() if k != "params"}
            merged = {**g, **hyper}
            merged["betas"] = hyper["betas"] = tuple(merged["betas"])
            if merged.get("amsgrad") or merged.get("maximize"):
                raise ValueError("FusedAdamW.load_state_dict: the saved optimiser used amsgrad / maximize, which are not implemented")
            self._check_group(merged)
            have = [(p, state_dict["state"][i]) for p, i in zip(g["params"], s["params"]) if i in state_dict["state"]]
            step = None
            if have:
                missing = [k for _, st in have for k in ("step", "exp_avg", "exp_avg_sq") if k not in st]
                if missing:
                    raise ValueError(f"FusedAdamW.load_state_dict: a saved parameter state lacks {sorted(set(missing))}")
                steps = {float(st["step"]) for _, st in have}
                if len(steps) != 1:
                    raise ValueError(f"FusedAdamW.load_state_dict: the parameters of group {gi} disagree on `step` ({sorted(steps)[:4]} ...): "
                                     "this optimiser keeps ONE applied-step count per group (every tensor of a group is updated in one call)")
                for p, st in have:
                    if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                        raise ValueError("FusedAdamW.load_state_dict: a saved moment has another shape than its parameter")
                step = steps.pop()
            plan.append((g, hyper, have, step))
        # nothing was refused: now change the optimiser
        self.state.clear()
        self._gstate = {}
        for gi, (g, hyper, have, step) in enumerate(plan):
            g.update(hyper)
            if not have:
                continue
            params = [p for p, _ in have]
            gs = self._group_state(gi, params[0].device)
            gs["step"].fill_(step)
            self._new_state(gs, params, [st["exp_avg"] for _, st in have], [st["exp_avg_sq"] for _, st in have])
        for post_hook in self._optimizer_load_state_dict_post_hooks.values():
            post_hook(self)
