#!/usr/bin/env python3
"""Record what the reference's two-stage validation (src/validate_blip_rerank.py: compute_cirr_val_metrics :165-248,
compute_fiq_val_metrics :23-83, both UNMODIFIED) returns on prepared stage-1 scores and a stage-2 probability table
-> tests/golden/rerank_val.npz (data only: the scores, the table, reference / target / group indices, the metric tuples).

Needs the reference checkout (oracle/ref_import.py); tests/test_rerank_val_gpu.py and tests/test_rerank_val_host.py need only
the file.   python tools/gen_rerank_val_golden.py

The fake dataset / fake model pattern is oracle/gen_golden.py's (metrics_goldens): `inference` returns rows of the prepared
`sim`, `inference_rerank` looks a probability table up by the image index that the fake "embeddings" carry (the index sits in
both entries of index_features: the reference's CIRR path takes candidates from [0], its FashionIQ path from [-1]).  The CIRR
function reads `sorted_index_names.npy` from the working directory (:195, a leftover that overwrites the order it has just
computed): it runs in a temporary directory holding the stable, reference-removed order (oracle.sprc_oracle.rank_stable) --
the array its own lines :186-193 compute on tie-free scores.  Scores and table are tie-free per row (asserted):
torch.argsort is not stable, a tie would make the reference's answer arbitrary.
"""
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import ref_import  # noqa: E402
from oracle import sprc_oracle as O  # noqa: E402

OUT = ROOT / "tests" / "golden" / "rerank_val.npz"
CIRR = dict(N=230, nq=37, top=200, seed=11)          # the reference's step = 15: blocks of 15, 15 and 7
FIQ = dict(N=97, nq=83, top=40, seed=8)             # step = 40: blocks of 40, 40 and 3
# stage-1 place of the target (CIRR: reference removed) -> its place after stage 2, one entry per repetition of the pattern:
# both sides of every K and of T; stage 2 moves targets across a K boundary in each direction; places >= T cannot move
CIRR_PLAN = {0: [2, 0, 7, 1], 4: [7, 2, 4, 12], 5: [3, 5, 0, 30], 9: [12, 4, 55, 9], 10: [0, 9, 10, 70], 49: [60, 3, 49, 120],
             50: [20, 49, 8, 50], 150: [8, 1, 45, 150], 199: [40, 199, 6, 0], 200: [200] * 4, 215: [215] * 4}
FIQ_PLAN = {9: [12, 3, 9, 30], 10: [5, 10, 38, 0], 39: [2, 39, 15, 8], 40: [40] * 4, 49: [49] * 4, 50: [50] * 4, 60: [60] * 4}


def import_rerank_harness():
    """src/validate_blip_rerank.py with the harness shims plus stubs for the two imports it never uses on this path."""
    ref_import.import_harness()
    clip = types.ModuleType("clip")
    clip.model = types.ModuleType("clip.model")
    clip.model.CLIP = object
    sys.modules["clip"], sys.modules["clip.model"] = clip, clip.model
    comb = types.ModuleType("combiner")
    comb.Combiner = object
    sys.modules["combiner"] = comb
    import importlib
    return importlib.import_module("validate_blip_rerank")


def tie_free(a: np.ndarray) -> bool:
    d = O.distances(a)
    return all(len(np.unique(r)) == len(r) for r in d)


def make_case(N, nq, top, seed, plan, remove_ref):
    """-> sim[nq,N], table[nq,N], ref, tgt, groups[nq,6]: targets at the planned stage-1 places, table rows that put them at the
    planned stage-2 places among the first T = top candidates."""
    rng = np.random.default_rng(seed)
    sim = rng.uniform(-0.2, 0.9, size=(nq, N)).astype(np.float32)
    table = rng.uniform(0.02, 0.98, size=(nq, N)).astype(np.float32)
    ref = rng.integers(0, N, size=nq)
    order = O.rank_stable(sim)
    places = sorted(plan)
    tgt = np.zeros(nq, dtype=np.int64)
    groups = np.zeros((nq, 6), dtype=np.int64)
    for q in range(nq):
        o = order[q][order[q] != ref[q]] if remove_ref else order[q]
        p1 = places[q % len(places)]
        if not remove_ref and o[p1] == ref[q]:                         # keep reference and target distinct
            ref[q] = o[(p1 + 7) % N]
        tgt[q] = o[p1]
        p2 = plan[p1][(q // len(places)) % 4]
        if p1 < top:                                                   # stage 2: a descending ladder over the first T candidates
            others = [int(i) for i in rng.permutation(o[:top]) if i != tgt[q]]
            ladder = others[:p2] + [int(tgt[q])] + others[p2:]
            vals = np.sort(rng.uniform(0.02, 0.98, size=top).astype(np.float32))[::-1]
            table[q, ladder] = vals
        rest = [i for i in rng.permutation(N) if i != ref[q] and i != tgt[q]][:4]
        groups[q] = rng.permutation(np.array([ref[q], tgt[q], *rest]))
    assert tie_free(sim) and tie_free(table), "scores and table must be tie-free per row"
    return sim, table, ref, tgt, groups


def main():
    vbr = import_rerank_harness()
    from torch.utils.data import Dataset

    class FakeModel:
        device = torch.device("cpu")

        def __init__(self, sim, table):
            self.sim, self.table = torch.from_numpy(sim), torch.from_numpy(table)

        def inference(self, reference_embeds, target_feats, captions):
            return self.sim[[int(c[1:]) for c in captions]]

        def inference_rerank(self, reference_feats, target_feats, captions):
            rows = torch.tensor([int(c[1:]) for c in captions])
            cand = target_feats.view(len(rows), -1).long()
            return self.table[rows[:, None], cand].reshape(-1)

    class CirrVal(Dataset):
        def __init__(self, names, ref, tgt, groups):
            self.names, self.ref, self.tgt, self.groups = names, ref, tgt, groups

        def __len__(self):
            return len(self.ref)

        def __getitem__(self, i):
            return self.names[self.ref[i]], self.names[self.tgt[i]], f"q{i}", [self.names[g] for g in self.groups[i]]

    class FiqVal(CirrVal):
        dress_types = ["dress"]

        def __getitem__(self, i):     # two captions; the fake processor below recovers the index from "Q<i> and x"
            return self.names[self.ref[i]], self.names[self.tgt[i]], [f"q{i}", "x"]

    out = {}
    # ---- CIRR ----
    c = CIRR
    sim, table, ref, tgt, groups = make_case(c["N"], c["nq"], c["top"], c["seed"], CIRR_PLAN, remove_ref=True)
    names = [f"img-{i:05d}" for i in range(c["N"])]
    index = torch.arange(c["N"], dtype=torch.float32).unsqueeze(1)
    order = O.rank_stable(sim)
    order = order[order != ref[:, None]].reshape(c["nq"], c["N"] - 1)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as d:
        np.save(Path(d) / "sorted_index_names.npy", np.array(names)[order])
        os.chdir(d)
        try:
            cirr = vbr.compute_cirr_val_metrics(CirrVal(names, ref, tgt, groups), FakeModel(sim, table), (index, index), names,
                                                {"eval": lambda s: s})
        finally:
            os.chdir(cwd)
    stage1 = O.cirr_metrics(sim, ref, tgt, groups)
    place = (order == tgt[:, None]).argmax(1)
    assert (place >= c["top"]).any() and (place < c["top"]).any(), "targets on both sides of T"
    assert all(a != b for a, b in zip(cirr, stage1)), f"every CIRR metric must move: {cirr} vs {stage1}"
    print("cirr  stage 1", [round(x, 3) for x in stage1], "\n      reranked", [round(x, 3) for x in cirr])
    out.update(cirr_sim=sim, cirr_table=table, cirr_ref=ref, cirr_tgt=tgt, cirr_groups=groups, cirr_top=np.int64(c["top"]),
               cirr_metrics=np.asarray(cirr, dtype=np.float64), cirr_stage1=np.asarray(stage1, dtype=np.float64))
    # ---- FashionIQ ----
    c = FIQ
    sim, table, ref, tgt, groups = make_case(c["N"], c["nq"], c["top"], c["seed"], FIQ_PLAN, remove_ref=False)
    names = [f"img-{i:05d}" for i in range(c["N"])]
    index = torch.arange(c["N"], dtype=torch.float32).unsqueeze(1)
    fiq = vbr.compute_fiq_val_metrics(FiqVal(names, ref, tgt, groups), FakeModel(sim, table), (index, index), names,
                                      {"eval": lambda s: "q" + s.split(" ")[0][1:]})
    stage1 = O.fiq_metrics(sim, tgt)
    place = (O.rank_stable(sim) == tgt[:, None]).argmax(1)
    assert (place >= c["top"]).any() and (place < c["top"]).any(), "targets on both sides of T"
    # Recall@50 cannot move: top = 40 < 50, a target among the first 40 stays there and one beyond keeps its place
    assert fiq[0] != stage1[0] and fiq[1] == stage1[1], f"FashionIQ Recall@10 must move: {fiq} vs {stage1}"
    print("fiq   stage 1", stage1, " reranked", fiq)
    out.update(fiq_sim=sim, fiq_table=table, fiq_ref=ref, fiq_tgt=tgt, fiq_top=np.int64(c["top"]),
               fiq_metrics=np.asarray(fiq, dtype=np.float64), fiq_stage1=np.asarray(stage1, dtype=np.float64))
    np.savez_compressed(OUT, **out)
    assert not any(v.dtype == object for v in np.load(OUT, allow_pickle=False).values())
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
