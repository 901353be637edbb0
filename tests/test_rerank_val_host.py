"""Two-stage validation, the parts that need no GPU: the two new entry points are declared, bound and documented; the golden of
the reference's validate_blip_rerank.py (tests/golden/rerank_val.npz, tools/gen_rerank_val_golden.py) loads, has the stated
shapes, and still shows what its generator asserted -- targets on both sides of T and metrics that differ from stage 1."""
import re
from pathlib import Path

import numpy as np
import pytest

from oracle import sprc_oracle as O
from sprc_amd import _lib

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("sprc_topk_wide", "sprc_rerank_order")


def test_header_binding_and_docs_name_both_functions():
    header = (ROOT / "include" / "sprc.h").read_text()
    for name in NAMES:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SIGNATURES
        for doc in ("DESIGN.md", "INTEGRATION.md"):
            assert name in (ROOT / doc).read_text(), (name, doc)
    assert len(_lib.SIGNATURES["sprc_topk_wide"][1]) == 11 and len(_lib.SIGNATURES["sprc_rerank_order"][1]) == 10
    assert _lib.ABI_VERSION == 8 == int(re.search(r"#define SPRC_ABI_VERSION (\d+)", header).group(1))
    assert "--rerank" in (ROOT / "README.md").read_text()


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(golden_dir / "rerank_val.npz", allow_pickle=False)


def _tie_free(a):
    return all(len(np.unique(r)) == len(r) for r in O.distances(a))


def test_golden_shapes(golden):
    g = golden
    assert g["cirr_sim"].shape == g["cirr_table"].shape == (37, 230) and g["cirr_sim"].dtype == g["cirr_table"].dtype == np.float32
    assert g["cirr_ref"].shape == g["cirr_tgt"].shape == (37,) and g["cirr_groups"].shape == (37, 6)
    assert g["cirr_metrics"].shape == g["cirr_stage1"].shape == (7,) and int(g["cirr_top"]) == 200
    assert g["fiq_sim"].shape == g["fiq_table"].shape == (83, 97) and g["fiq_tgt"].shape == (83,)
    assert g["fiq_metrics"].shape == g["fiq_stage1"].shape == (2,) and int(g["fiq_top"]) == 40
    assert (ROOT / "tests" / "golden" / "rerank_val.npz").stat().st_size < 200 * 1024
    for k in ("cirr_sim", "cirr_table", "fiq_sim", "fiq_table"):       # torch.argsort is not stable: a tie would make the reference arbitrary
        assert _tie_free(g[k]), k


def test_golden_targets_sit_at_the_planted_ranks_and_the_rerank_moves_every_metric(golden):
    g = golden
    order = O.rank_stable(g["cirr_sim"])
    order = order[order != g["cirr_ref"][:, None]].reshape(37, 229)
    place = (order == g["cirr_tgt"][:, None]).argmax(1)
    assert set(place.tolist()) == {0, 4, 5, 9, 10, 49, 50, 150, 199, 200, 215}          # both sides of every K and of T = 200
    stage1 = O.cirr_metrics(g["cirr_sim"], g["cirr_ref"], g["cirr_tgt"], g["cirr_groups"])
    assert stage1 == tuple(g["cirr_stage1"].tolist())
    assert all(a != b for a, b in zip(g["cirr_metrics"].tolist(), stage1))
    place = (O.rank_stable(g["fiq_sim"]) == g["fiq_tgt"][:, None]).argmax(1)
    assert set(place.tolist()) == {9, 10, 39, 40, 49, 50, 60}                            # T = 40
    stage1 = O.fiq_metrics(g["fiq_sim"], g["fiq_tgt"])
    assert stage1 == tuple(g["fiq_stage1"].tolist())
    # Recall@50 cannot move with top = 40: a target among the first 40 stays there, one beyond keeps its place
    assert g["fiq_metrics"][0] != stage1[0] and g["fiq_metrics"][1] == stage1[1]
    # stage 2 moves targets across a K boundary in each direction
    t = g["cirr_table"]
    new = np.array([(np.argsort(np.float32(1) - t[q, order[q, :200]], kind="stable") == p).argmax() if p < 200 else p
                    for q, p in enumerate((order == g["cirr_tgt"][:, None]).argmax(1))])
    old = (order == g["cirr_tgt"][:, None]).argmax(1)
    for K in (1, 5, 10, 50):
        assert ((old < K) & (new >= K)).any() and ((old >= K) & (new < K)).any(), K


def test_rerank_under_torchrun_is_refused(monkeypatch):
    from sprc_amd import blip_validate as bv
    monkeypatch.setenv("WORLD_SIZE", "2")
    for ds in ("CIRR", "fashionIQ"):
        with pytest.raises(SystemExit, match="--rerank runs on one process"):
            bv.main(["--dataset", ds, "--model-path", "none.pt", "--rerank", "true"])
    with pytest.raises(SystemExit, match="CIRR and fashionIQ"):
        bv.main(["--dataset", "CIRCO", "--model-path", "none.pt", "--rerank", "true"])
