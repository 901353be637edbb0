"""Every attention kernel path at wide softmax logit ranges, against a float64 softmax of the same rounded operands.

The other attention tests draw q, k, v from N(0, 1): scores of about N(0, 1), so after the first 32-key tile the running max of the online
softmax never moves.  Here (tests/_attn_logits.py) the rows of every 32-query tile carry different logit patterns -- early peaks with gaps of
3 / 20 / 60 nats, late keys 5.3 / 5.8 / 15 / 40 nats above tile 0's max (either side of the streaming kernels' lazy-rescale threshold of
8 log2 units, and past fp16's range of P had that threshold been above 16) in a middle tile, the last full tile, a ragged last tile of
either kind and both ends of a second key segment, staircases of 5 and 6 nats per tile, +-50 nat offsets -- and, where the path takes a
key mask, the first one or two tiles, the would-be peak, or all keys but one masked.  tests/test_attn_logits.py checks on the host that
the patterns came out as intended; each case lists its path (the kernel sprc_attention picks for the shape: attention16 in
sprc_amd/csrc/attention.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _attn_logits as A  # noqa: E402
from sprc_amd import engine as E  # noqa: E402

DEV = "cuda:0"
TOL = {"bf16": 2e-2, "fp16": 2e-3, "f32": 2e-5}      # the suite's bars for the three operand types
CASES = [(sid, path, dt, kw, x3) for sid, path, dts, kw, x3 in A.SPECS for dt in dts]


def _compare(c, got, want, tol, what):
    """assert_close(got, want, atol=tol, rtol=tol) that names the row patterns that broke it"""
    got = got.double().view(c.B, c.Tq, c.H, c.dh)
    bad = ~((got - want).abs() <= tol + tol * want.abs())            # NaN / inf fail too
    if bool(bad.any()):
        rows = bad.any(-1).permute(0, 2, 1)                           # [B, H, Tq]
        names = sorted({c.pats[int(p)].name for p in c.row_pat[rows]})
        kinds = sorted(set(c.mask_kinds[b] for b in rows.nonzero()[:, 0].tolist())) if c.mask_kinds else []
        err = float(torch.nan_to_num((got - want).abs(), nan=float("inf")).max())
        pytest.fail(f"{what}: {int(rows.sum())} of {rows.numel()} rows off by more than {tol} (max err {err:.3g}); "
                    f"patterns {names}" + (f", masks {kinds}" if kinds else ""))


def _attention(c, dev, out_x3=False):
    D = c.H * c.dh
    kw = {}
    if c.Tk2:
        kw.update(k2=dev["kb"], v2=dev["vb"], Tk2=c.Tk2, ld2=D)
    return E.attention(dev["q"], dev["ka"], dev["va"], c.B, c.H, c.Tq, c.Tk1, c.dh, D, D, D, c.scale, key_mask=dev.get("mask"),
                       kv_index=dev.get("ia"), kv2_index=dev.get("ib"), out_x3=out_x3, **kw)


@pytest.mark.parametrize("sid,path,dtype,kw,x3", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_attention_at_wide_logit_ranges(sid, path, dtype, kw, x3):
    c = A.case_for(sid, kw, dtype)
    dev = {n: getattr(c, n) for n in ("q", "ka", "va", "kb", "vb") if getattr(c, n) is not None}
    dev = {n: c.flat(t).to(DEV) for n, t in dev.items()}
    for n in ("ia", "ib", "mask"):
        if getattr(c, n) is not None:
            dev[n] = getattr(c, n).to(DEV)
    want = c.reference()
    out = _attention(c, dev)
    assert out.dtype == c.q.dtype
    _compare(c, out.cpu(), want, TOL[dtype], f"{sid} {dtype} ({path})")
    if x3 and dtype == "fp16":
        # split-precision output rows (SPRC_F16X3) written straight from the registers: hi + lo carries the fp32 result
        hi, lo8, _ = E.split_decode(_attention(c, dev, out_x3=True).cpu(), c.H * c.dh)
        _compare(c, hi.double() + lo8.double(), want, TOL[dtype], f"{sid} {dtype} ({path}, split output hi + lo)")


@pytest.mark.parametrize("sid,kw", A.BWD_SPECS, ids=[s[0] for s in A.BWD_SPECS])
def test_attention_backward_at_wide_logit_ranges(sid, kw):
    """sprc_attention_bwd (fp32, head_dim 64) on the same patterns: dq, dk, dv against torch.autograd in float64."""
    from sprc_amd import train as T
    c = A.case_for(sid, kw, "f32")
    B, H, Tq, Tk, dh = c.B, c.H, c.Tq, c.Tk, c.dh
    do = torch.randn((B, Tq, H, dh), generator=torch.Generator().manual_seed(17))
    qq, kk, vv = (t.double().requires_grad_(True) for t in (c.q, c.ka, c.va))
    s = torch.einsum("bqhd,bkhd->bhqk", qq, kk) * c.scale
    if c.mask is not None:
        s = s + c.mask.double()[:, None, None, :]
    torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), vv).backward(do.double())
    k = T._K(torch.device(DEV))
    md = None if c.mask is None else c.mask.to(DEV)
    dq, dk, dv = k.attention_bwd(c.flat(c.q).to(DEV), c.flat(c.ka).to(DEV), c.flat(c.va).to(DEV), c.flat(do).to(DEV), B, H, Tq, Tk, md, c.scale)
    for name, got, want, T_ in (("dq", dq, qq.grad, Tq), ("dk", dk, kk.grad, Tk), ("dv", dv, vv.grad, Tk)):
        got = got.cpu().double().view(B, T_, H, dh)
        torch.testing.assert_close(got, want, atol=3e-5, rtol=0, msg=lambda m: f"{sid} {name}\n{m}")
