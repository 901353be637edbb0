"""Two-stage validation on the GPU (validate_blip_rerank.py): sprc_rerank_order against a numpy model; the CIRR / FashionIQ
metrics after the rerank against the tuples the UNMODIFIED reference returned on the same scores and probability table
(tests/golden/rerank_val.npz, tools/gen_rerank_val_golden.py) and, where `top` exceeds the gallery, against a numpy restatement;
one end-to-end case on real stage-2 scores; `blip_validate --rerank true` on the on-disk synthetic tree."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sprc_oracle as O  # noqa: E402
from sprc_amd import engine as E  # noqa: E402
from sprc_amd import harness as H  # noqa: E402
from sprc_amd import synth  # noqa: E402
from sprc_amd._lib import SprcError  # noqa: E402
from sprc_amd.config import get_config  # noqa: E402
from sprc_amd.model import Blip2QformerCirRerank  # noqa: E402
from test_entrypoints_gpu import DEPTH, _oracle_metrics, world  # noqa: E402,F401  (the on-disk synthetic tree and its independent evaluation)
from test_rerank_gpu import _Tok  # noqa: E402

DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent


# ---- sprc_rerank_order -----------------------------------------------------------------------------------------------------------
def order_model(cand, prob, listed, listed_rank):
    """numpy model: real candidates by the stable argsort of fl32(1 - prob), padding after them as -1; listed items take their
    new position when they are candidates of the row."""
    nq, T = cand.shape
    out_idx = np.full((nq, T), -1, dtype=np.int32)
    out_rank = np.full(listed.shape, -1, dtype=np.int32)
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            d = np.float32(1) - prob[q].astype(np.float32)
        perm = [p for p in np.argsort(d, kind="stable") if cand[q, p] >= 0]
        out_idx[q, :len(perm)] = cand[q, perm]
        for l in range(listed.shape[1]):
            g = listed[q, l]
            if g >= 0:
                hit = np.nonzero(out_idx[q] == g)[0]
                out_rank[q, l] = hit[0] if len(hit) else listed_rank[q, l]
    return out_idx, out_rank


@pytest.mark.parametrize("T", [1, 2, 40, 63, 64, 65, 200, 256])
def test_rerank_order_against_numpy(T):
    rng = np.random.default_rng(T)
    nq = 7
    cand = np.stack([10 + rng.permutation(990)[:T] for _ in range(nq)]).astype(np.int32)
    if T > 2:
        cand[:, 1] = 3                                                    # one item that every query has and lists
    prob = rng.uniform(0.01, 0.99, size=(nq, T)).astype(np.float32)
    prob[1] = np.round(prob[1] * 8) / 8                                   # tied probabilities: stage-1 order decides
    prob[2] = 0.5
    prob[3, T // 2] = np.nan                                              # a NaN candidate is the last REAL one
    prob[0, 0], prob[0, -1] = 1.0, 0.0
    cand[4, T - 1:] = -1                                                  # padding tails of length 1 and T - 1,
    cand[5, 1:] = -1                                                      # whatever their prob
    prob[5, 1:] = 2.0
    cand[6, T // 3] = -1                                                  # (and a hole, which the contract also calls padding)
    for L in (0, 1, 7, 16):
        listed = np.full((nq, L), -1, dtype=np.int32)
        for q in range(nq):
            want = [cand[q, 0], cand[q, T - 1], 5000 + q, -1, 3, cand[q, T // 2], cand[q, min(1, T - 1)]]
            want += [int(x) for x in rng.integers(0, 1000, size=16)]
            listed[q] = want[:L]
        listed_rank = rng.integers(T, 5000, size=(nq, L)).astype(np.int32)
        got_idx, got_rank = E.rerank_order(torch.from_numpy(cand).to(DEV), torch.from_numpy(prob).to(DEV),
                                           torch.from_numpy(listed), torch.from_numpy(listed_rank))
        want_idx, want_rank = order_model(cand, prob, listed, listed_rank)
        assert np.array_equal(got_idx.cpu().numpy(), want_idx), (T, L)
        assert np.array_equal(got_rank.cpu().numpy(), want_rank), (T, L)
    only_idx, none = E.rerank_order(torch.from_numpy(cand).to(DEV), torch.from_numpy(prob).to(DEV))
    assert np.array_equal(only_idx.cpu().numpy(), want_idx) and none.shape == (nq, 0)


def test_rerank_order_bad_arguments():
    cand = torch.zeros((2, 257), dtype=torch.int32, device=DEV)
    with pytest.raises(SprcError, match="sprc_rerank_order"):
        E.rerank_order(cand, torch.zeros((2, 257), device=DEV))
    with pytest.raises(SprcError, match="sprc_rerank_order"):
        E.rerank_order(cand[:, :8].contiguous(), torch.zeros((2, 8), device=DEV), torch.zeros((2, 17), dtype=torch.int32),
                       torch.zeros((2, 17), dtype=torch.int32))


# ---- the metrics after the rerank ---------------------------------------------------------------------------------------------------
def rerank_places(sim, ref, listed, prob_of, top):
    """numpy restatement of the rule: stable order by (fl32(1 - sim), index), the reference dropped when `ref` is given, the first
    T = min(top, entries) re-ordered by the stable argsort of fl32(1 - P), the rest in place -> position of every listed item
    (-1: not in the order)."""
    order = O.rank_stable(sim)
    nq = len(order)
    place = np.full(listed.shape, -1, dtype=np.int64)
    for q in range(nq):
        o = order[q][order[q] != ref[q]] if ref is not None else order[q].copy()
        T = min(top, len(o))
        p = np.asarray(prob_of(q, o[:T]), dtype=np.float32)
        o[:T] = o[:T][np.argsort(np.float32(1) - p, kind="stable")]
        for l, g in enumerate(listed[q]):
            hit = np.nonzero(o == g)[0]
            if g >= 0 and len(hit):
                place[q, l] = hit[0]
    return place


def cirr_restated(sim, ref, tgt, grp, prob_of, top):
    place = rerank_places(sim, ref, np.concatenate([tgt[:, None], grp], axis=1), prob_of, top)
    r_t, r_g = place[:, 0], place[:, 1:]
    before = ((r_g < r_t[:, None]) & (r_g >= 0)).sum(1)
    return tuple(H._pct(before < k) for k in (1, 2, 3)) + tuple(H._pct(r_t < k) for k in (1, 5, 10, 50))


def fiq_restated(sim, tgt, prob_of, top):
    r = rerank_places(sim, None, tgt[:, None], prob_of, top)[:, 0]
    return H._pct(r < 10), H._pct(r < 50)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "rerank_val.npz", allow_pickle=False)


def table_fn(table: np.ndarray, on_device: bool):
    t = torch.from_numpy(table).to(DEV if on_device else "cpu")

    def rerank_fn(rows, cand):
        assert cand.dtype == torch.int64 and cand.shape[0] == len(rows)
        return t[torch.tensor(rows, device=t.device)[:, None], cand.to(t.device)]
    return rerank_fn


def test_cirr_metrics_after_rerank_equal_the_reference(golden):
    g = golden
    sim = torch.from_numpy(g["cirr_sim"]).to(DEV)
    got = H.cirr_rerank_metrics_from_sim(sim, g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], table_fn(g["cirr_table"], True))
    assert got == tuple(g["cirr_metrics"].tolist())
    assert all(a != b for a, b in zip(got, g["cirr_stage1"].tolist()))                  # the second stage really re-orders
    assert H.cirr_rerank_metrics_from_sim(sim, g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], table_fn(g["cirr_table"], False),
                                          top=int(g["cirr_top"])) == got           # probabilities from the host: the same
    assert got == cirr_restated(g["cirr_sim"], g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], lambda q, c: g["cirr_table"][q, c], 200)
    # `top` beyond the gallery clamps to N - 1 (the reference's reshape(-1, top) breaks there); other sizes of the first stage
    for top in (256, 1, 64, 65):
        assert H.cirr_rerank_metrics_from_sim(sim, g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], table_fn(g["cirr_table"], True), top=top) == \
            cirr_restated(g["cirr_sim"], g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], lambda q, c: g["cirr_table"][q, c], top), top
    with pytest.raises(ValueError):
        H.cirr_rerank_metrics_from_sim(sim.repeat(1, 2), g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"], table_fn(g["cirr_table"], True),
                                       top=300)           # 300 of 459 entries: beyond what the kernels re-order
    # a group member that is missing from the gallery never counts (as in cirr_metrics_from_sim)
    grp = g["cirr_groups"].copy()
    grp[np.arange(len(grp)), (grp != g["cirr_tgt"][:, None]).argmax(1)] = -1
    assert H.cirr_rerank_metrics_from_sim(sim, g["cirr_ref"], g["cirr_tgt"], grp, table_fn(g["cirr_table"], True)) == \
        cirr_restated(g["cirr_sim"], g["cirr_ref"], g["cirr_tgt"], grp, lambda q, c: g["cirr_table"][q, c], 200)


def test_fiq_metrics_after_rerank_equal_the_reference(golden):
    g = golden
    sim = torch.from_numpy(g["fiq_sim"]).to(DEV)
    got = H.fiq_rerank_metrics_from_sim(sim, g["fiq_tgt"], table_fn(g["fiq_table"], True))
    assert got == tuple(g["fiq_metrics"].tolist())
    assert got[0] != g["fiq_stage1"][0]
    for top in (40, 256, 97, 1, 10):          # 256 > N = 97: clamps
        assert H.fiq_rerank_metrics_from_sim(sim, g["fiq_tgt"], table_fn(g["fiq_table"], False), top=top) == \
            fiq_restated(g["fiq_sim"], g["fiq_tgt"], lambda q, c: g["fiq_table"][q, c], top), top


# ---- real stage-2 scores -------------------------------------------------------------------------------------------------------------
def test_two_stage_cirr_on_real_stage2_scores():
    """ViT-L depth 1, fp32, 12 images, 5 queries, top = 6: the recorded stage-2 probabilities are the oracle's within the fp32
    tolerance of tests/test_rerank_gpu.py (2e-5), and the metrics are the numpy restatement applied to the engine's OWN scores and
    probabilities (a 2e-5 difference may legitimately swap near-equal candidates, so the order is not held to the oracle's)."""
    cfg = get_config("pretrain_vitL", vit_depth=1)
    sd = synth.make_state_dict(cfg, seed=41)
    n_img, nq, top = 12, 5, 6
    images = synth.make_images(n_img, seed=42)
    ids, mask, ref = synth.make_queries(nq, n_img, seed=43)
    model = Blip2QformerCirRerank(cfg=cfg, compute_dtype="fp32", max_batch=8)
    assert not model.load_state_dict(sd, strict=False).missing_keys
    model = model.to(DEV)
    model.tokenizer = _Tok(ids, mask)
    caps = [f"q{i}" for i in range(nq)]
    feats, raw = model.extract_target_features(images.to(DEV))
    sim = model.inference(raw[ref.to(DEV)], feats, caps)
    names = [f"img-{i:02d}" for i in range(n_img)]
    ref_np = ref.numpy()
    tgt = (ref_np + 1 + np.arange(nq)) % n_img
    rng = np.random.default_rng(44)
    grp = np.stack([rng.permutation([ref_np[q], tgt[q], *[i for i in rng.permutation(n_img) if i not in (ref_np[q], tgt[q])][:4]])
                    for q in range(nq)])
    inner = H.make_rerank_fn(model, names, dict(zip(names, raw)), [names[r] for r in ref_np], ref_np.tolist(), caps)
    seen = {}

    def rerank_fn(rows, cand):
        p = inner(rows, cand)
        for i, q in enumerate(rows):
            seen[q] = (cand[i].cpu().numpy(), p[i].cpu().numpy())
        return p

    got = H.cirr_rerank_metrics_from_sim(sim, ref_np, tgt, grp, rerank_fn, top=top)
    assert sorted(seen) == list(range(nq)) and all(len(c) == top for c, _ in seen.values())
    sim_np = sim.cpu().numpy()
    for q, (c, _) in seen.items():                                        # the candidates: the reference-less stage-1 order
        o = O.rank_stable(sim_np[q:q + 1])[0]
        assert np.array_equal(c, o[o != ref_np[q]][:top])
    cand = torch.from_numpy(np.stack([seen[q][0] for q in range(nq)]))
    with torch.no_grad():
        raw_o = O.encode_image_tokens(sd, cfg, images)
        want = O.inference_rerank(sd, cfg, raw_o[ref], raw_o[cand.reshape(-1)], ids, mask).numpy().reshape(nq, top)
    have = np.stack([seen[q][1] for q in range(nq)])
    print(f"\n[two-stage, fp32] max|dprob| = {np.abs(have - want).max():.2e}")
    np.testing.assert_allclose(have, want, atol=2e-5, rtol=0)

    def prob_of(q, c):
        assert np.array_equal(c, seen[q][0])
        return seen[q][1]
    assert got == cirr_restated(sim_np, ref_np, tgt, grp, prob_of, top)


# ---- the entry point -------------------------------------------------------------------------------------------------------------------
KEYS = ("group_recall_at1", "group_recall_at2", "group_recall_at3", "recall_at1", "recall_at5", "recall_at10", "recall_at50")


def test_blip_validate_rerank_on_disk(world, capsys):
    args = ["--dataset", "CIRR", "--model-path", str(world["root"] / "ckpt.pt"), "--dtype", "fp32", "--vit-depth", str(DEPTH)]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-m", "sprc_amd.blip_validate", *args, "--rerank", "true"],
                         cwd=ROOT, env=dict(os.environ), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "reranking now" in run.stdout
    out = json.loads(run.stdout[run.stdout.rindex("{"):])
    vals = [out[k] for k in KEYS]
    assert all(isinstance(v, float) and math.isfinite(v) and 0.0 <= v <= 100.0 for v in vals), out
    # without the flag: what it printed before -- the independent evaluation of the same files
    from sprc_amd import blip_validate as bv
    plain = bv.main(args)
    sim, ref, tgt, grp = _oracle_metrics(world)
    assert tuple(plain[k] for k in KEYS) == pytest.approx(O.cirr_metrics(sim, ref, tgt, grp), abs=1e-4)
    assert "reranking now" not in capsys.readouterr().out
    assert set(plain) == set(out)                                                  # the same metric lines
