"""References and buffers of tests/test_train_kernels_gpu.py: every backward kernel of csrc/train.hip alone.

Three things live here and nothing else:
  * `Guard` -- a sentinel-filled allocation that hands out strided logical views (`ld > width`, packed column slices, an exact-size
    workspace at an aligned offset) and afterwards proves, bit for bit, that nothing outside those views changed;
  * the operations written plainly in torch (float64 on the CPU, autograd for the gradients; the same functions at float32 give the
    "what does a plain fp32 evaluation lose" yardstick) -- never another kernel of the library;
  * the two numerical bars: `sum_bound` (outputs that are a plain sum of n fp32 terms) and `calibrated` (everything else: the kernel's
    error against fp64 at most 4 x the error of torch's own fp32 CPU evaluation of the same expression).
Nothing here is product code."""
from __future__ import annotations

import numpy as np
import torch

SENTINEL = -777.25                      # finite: an input that must not be read, an output that must not be written
U = 2.0 ** -24                          # unit roundoff of fp32


class Guard:
    """One flat allocation filled with `fill`; `view` / `matrix` mark the logical regions; `seal` after the inputs are in place,
    `outside_intact` after the call (all of it with `whole=True`: a read-only input)."""

    def __init__(self, numel, fill=SENTINEL, dtype=torch.float32, device="cpu"):
        self.buf = torch.full((int(numel),), fill, dtype=dtype, device=device)
        self._ix = torch.arange(int(numel), device=device)
        self.inside = torch.zeros(int(numel), dtype=torch.bool, device=device)
        self.snap = None

    def view(self, offset, shape, strides):
        self.inside[self._ix.as_strided(shape, strides, offset).reshape(-1)] = True
        return self.buf.as_strided(shape, strides, offset)

    def matrix(self, rows, cols, ld, offset=0):
        assert ld >= cols and offset + rows * ld <= self.buf.numel()
        return self.view(offset, (rows, cols), (ld, 1))

    def _bits(self, t):
        return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])

    def seal(self):
        self.snap = self.buf.clone()
        return self

    def outside_intact(self, whole=False):
        a, b = self._bits(self.buf), self._bits(self.snap)
        return bool(torch.equal(a, b)) if whole else bool(torch.equal(a[~self.inside], b[~self.inside]))


LEAD = 8                                # elements in front of every logical region (32 bytes of fp32: 16-byte alignment is kept)


def strided(rows, cols, ld, fill=SENTINEL, dtype=torch.float32, device="cpu", data=None):
    """(guard, logical [rows, cols] view with leading dimension ld) with LEAD sentinel elements in front and behind; `data` is copied in."""
    g = Guard(LEAD + rows * ld + LEAD, fill, dtype, device)
    v = g.matrix(rows, cols, ld, LEAD)
    if data is not None:
        v.copy_(data.to(dtype).reshape(rows, cols))
    return g, v


# ---- the two bars ---------------------------------------------------------------------------------------------------------------
def sum_bound(n, abs_terms, ref):
    """Forward error bound of a sum / dot product of n fp32 terms, any order, with a factor 2 of slack:
    2 n 2^-24 sum|term_i|, plus one ulp of the result for the final rounding.  All float64."""
    return 2.0 * n * U * abs_terms + 2.0 ** -23 * ref.abs() + 1e-45


def assert_sum_bound(what, got, ref, n, abs_terms):
    err = (got.double().cpu() - ref).abs()
    bound = sum_bound(n, abs_terms, ref)
    worst = float((err / bound).max())
    print(f"[{what}] max |kernel - fp64| = {float(err.max()):.3e}, worst error / bound = {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (what, float(err.max()), worst)


RATIOS = {}                             # kernel output -> largest e_kernel / e_torch seen in this session (printed by the last test)


def calibrated(what, got, ref64, ref32, key=None, scale=None):
    """e_kernel = max|kernel - fp64| <= 4 x e_torch = max|torch fp32 CPU - fp64| on the same inputs.  The factor 4 is for the kernels'
    reduction order (64-lane butterflies, per-wave partials) against torch's vectorised CPU code.  e_torch is floored at half an ulp of
    the output's largest magnitude (2^-24 max|ref|): on tiny cases torch's evaluation happens to be exact, and no fp32 result that
    went through one rounding at that magnitude can be held to less.  `scale` replaces max|ref| in the floor where the output is a
    DIFFERENCE that can cancel completely (then the terms' magnitude, given by the caller, is what one rounding is measured against)."""
    got, ref64, ref32 = (torch.as_tensor(t).double().cpu().reshape(-1) for t in (got, ref64, ref32))
    assert bool(torch.isfinite(got).all()), what
    e_k, e_t = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    floor = U * float(ref64.abs().max() if scale is None else scale)
    bar = 4.0 * max(e_t, floor)
    ratio = e_k / max(e_t, floor) if max(e_t, floor) > 0 else (0.0 if e_k == 0 else float("inf"))
    print(f"[{what}] max |kernel - fp64| = {e_k:.3e}, max |torch fp32 - fp64| = {e_t:.3e} (floor {floor:.1e}), ratio {ratio:.2f}")
    if key is not None:
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert e_k <= bar, (what, e_k, e_t, floor)
    return ratio


# ---- the operations, plainly ----------------------------------------------------------------------------------------------------
def grads_of(fn, inputs, dout, dtype):
    """(output, gradients of sum(output * dout) with respect to every input) of fn at `dtype` on the CPU"""
    xs = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    y = fn(*xs)
    gs = torch.autograd.grad(y, xs, dout.to(dtype).reshape(y.shape), allow_unused=True)
    return y.detach(), [torch.zeros_like(x) if g is None else g for x, g in zip(xs, gs)]


def gelu(x):
    return torch.nn.functional.gelu(x)


def layer_norm(eps):
    return lambda x, gamma, beta: torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma, beta, eps)


def attention(B, H, Tq, Tk, scale, mask, keep, drop_scale):
    """q [B*Tq, H*64], k / v [B*Tk, H*64] -> [B*Tq, H*64]: ((keep / (1 - p)) o softmax(q k^T scale + mask)) v.
    mask [B, Tk] or None, keep [B, H, Tq, Tk] bool or None."""
    def fn(q, k, v):
        s = torch.einsum("bqhd,bkhd->bhqk", q.view(B, Tq, H, 64), k.view(B, Tk, H, 64)) * scale
        if mask is not None:
            s = s + mask.to(q.dtype)[:, None, None, :]
        p = torch.softmax(s, -1)
        if keep is not None:
            p = p * keep.to(q.dtype) * torch.tensor(drop_scale, dtype=q.dtype)
        return torch.einsum("bhqk,bkhd->bqhd", p, v.view(B, Tk, H, 64)).reshape(B * Tq, H * 64)
    return fn


def embed_rows(ids, B, Lq, Lt, vocab, no_img, shared):
    """query [Lq, h] (shared) or [B, Lq, h], word [vocab, h], pos [P, h] -> pre [B, Lq + Lt, h].  Ids are clamped to [0, vocab) as the
    kernels clamp them, forward and backward alike.  Image mode: [query rows | word + pos[0..Lt)]; text-only mode:
    [word(ids[:, 0]) | query rows | word(ids[:, 1:])] + pos[0..Lq+Lt)."""
    def fn(query, word, pos):
        q = query.unsqueeze(0).expand(B, Lq, -1) if shared else query
        if Lt == 0:
            return q + 0
        w = word[ids.clamp(0, vocab - 1)]
        if no_img:
            return torch.cat([w[:, :1], q, w[:, 1:]], 1) + pos[:Lq + Lt]
        return torch.cat([q, w + pos[:Lt]], 1)
    return fn


def first_argmax(s):
    """first maximal index over the last dimension, explicitly (no reliance on torch.max's tie rule)"""
    J = s.shape[-1]
    ismax = s == s.max(-1, keepdim=True).values
    return torch.where(ismax, torch.arange(J), torch.tensor(J)).min(-1).values


def contrastive_ce():
    def fn(sim, temp):
        return torch.nn.functional.cross_entropy(sim / temp, torch.arange(sim.shape[0]))
    return fn


def l2norm(x):
    return torch.nn.functional.normalize(x, dim=-1)                 # x / max(||x||, 1e-12)


def align_mse(h, prompt):
    """h [B, Lq, D], prompt [Lq, D]: mse(mean_j h, mean_j prompt); the prompt side is detached in the model"""
    return torch.nn.functional.mse_loss(h.mean(1), prompt.mean(0).expand(h.shape[0], -1))


def keep_mask(seed, site, shape, p):
    from oracle.sprc_oracle import drop_keep
    return torch.from_numpy(np.ascontiguousarray(drop_keep(seed, site, int(np.prod(shape)), p))).view(*shape)


def drop_scale(p):
    """the kernels' fp32 1 / (1 - p)"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
