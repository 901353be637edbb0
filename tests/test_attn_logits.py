"""Host check of the structured-logit attention inputs (tests/_attn_logits.py) that tests/test_attention_range_gpu.py feeds the kernels:
every pattern came out as intended in float64 from the rounded operands, so the GPU test cannot pass only because its construction went
wrong (a late key on the wrong side of the lazy-rescale threshold, a staircase that never climbs, a mask that leaves a row empty)."""
import math

import pytest
import torch

import _attn_logits as A

CASES = [(sid, path, dt, kw) for sid, path, dts, kw, _ in A.SPECS for dt in dts] + [(sid, "bwd", "f32", kw) for sid, kw in A.BWD_SPECS]


@pytest.mark.parametrize("sid,path,dtype,kw", CASES, ids=[f"{c[0]}-{c[2]}" for c in CASES])
def test_every_row_follows_its_pattern(sid, path, dtype, kw):
    c = A.case_for(sid, kw, dtype)
    bad = A.check_case(c)
    assert not bad, "\n".join(bad[:20])
    assert c.q.dtype == c.ka.dtype == c.va.dtype == {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}[dtype]
    # the reference is a softmax of finite logits over at least one key: finite, and a convex combination of v per row
    ref = c.reference()
    _, v = c.keys()
    assert torch.isfinite(ref).all()
    assert bool((ref <= v.amax(1, keepdim=True) + 1e-9).all() and (ref >= v.amin(1, keepdim=True) - 1e-9).all())


@pytest.mark.parametrize("sid,path,dtype,kw", [c for c in CASES if c[1] != "bwd"], ids=[f"{c[0]}-{c[2]}" for c in CASES if c[1] != "bwd"])
def test_each_spec_reaches_the_kernel_it_names(sid, path, dtype, kw):
    assert A.expected_path(kw, dtype) == path


def test_the_matrix_covers_every_pattern_where_the_kernels_branch():
    """Per path: late jumps on both sides of the threshold in a middle tile, the last full tile and a ragged last tile of both kinds
    (tail_small: <= 4 keys, generic), staircases and +-50 offsets; masks of every kind; fp16 and bf16 wherever the kernel is 16-bit."""
    seen = {}
    for sid, path, dts, kw, _ in A.SPECS:
        locs = A.locations(kw["Tk1"], kw.get("Tk2", 0))
        got = seen.setdefault(path, {"pats": set(), "tails": set(), "masks": set(), "dtypes": set()})
        got["pats"] |= {p.name.split("@")[0] + ("@" + p.loc if p.loc else "") for p in A.patterns(locs)}
        got["tails"].add(A.tail_kind(kw["Tk1"] + kw.get("Tk2", 0)))
        got["masks"] |= set(kw.get("masks", ()))
        got["dtypes"] |= set(dts)
    for path in ("stream1", "stream3"):
        assert seen[path]["tails"] == {"none", "small", "generic"}, path
        assert {f"late{j:g}@{loc}" for j in A.JUMPS for loc in ("mid", "lastfull", "tail")} <= seen[path]["pats"], path
    for path in ("res9", "res4", "res8", "f32"):
        assert seen[path]["masks"] == set(A.MASKS), path
    assert {f"late{j:g}@{loc}" for j in A.JUMPS for loc in ("seg2_first", "seg2_last")} <= seen["res4"]["pats"] & seen["f32"]["pats"]
    for path in ("stream1", "stream3", "res9", "res2", "res4", "res8"):
        assert seen[path]["dtypes"] == {"bf16", "fp16"}, path
        assert {"stair5", "stair6", "early3+50", "flat-50", "stair6-50"} <= seen[path]["pats"]
    # the jumps straddle the threshold of the lazy running max: 8 log2 units
    assert min(j for j in A.JUMPS if j > A.RESCALE_NATS) - A.RESCALE_NATS > 0.2 and A.RESCALE_NATS - max(j for j in A.JUMPS if j < A.RESCALE_NATS) > 0.2
    assert any(j * math.log2(math.e) > 16 for j in A.JUMPS)          # fp16 P would overflow were the threshold above 16 log2
