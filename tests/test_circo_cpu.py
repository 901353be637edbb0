"""CIRCO without a GPU: the dataset class against what the reference's class yields over the same synthetic tree
(tests/golden/circo_items.json, recorded by tools/gen_circo_golden.py), the host-side metric of the sharded path against a
brute-force numpy evaluation, and the sharded CIRCO evaluation on 2 and 3 gloo ranks (oracle-backed doubles, as in
tests/test_dist_eval_cpu.py) against the single-process numbers."""
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, str(Path(__file__).resolve().parent))

import _circo_tree as CT  # noqa: E402
import _dist_case as DC  # noqa: E402

KS = (5, 10, 25, 50)


# ---- the metric, brute force: a full stable argsort and precision at every hit, in float64 ------------------------------------
def brute_circo(sim, gt_lists, tgt_idx):
    """gt_lists: per query the DISTINCT ground-truth gallery indices.  -> the eight numbers and the per-query AP table."""
    d = np.float32(1.0) - np.asarray(sim, dtype=np.float32)
    order = np.argsort(d, axis=1, kind="stable")
    ap = np.zeros((len(order), len(KS)), dtype=np.float64)
    rec = np.zeros((len(order), len(KS)), dtype=np.float64)
    for q, row in enumerate(order):
        gts = set(int(g) for g in gt_lists[q])
        for j, K in enumerate(KS):
            hits, acc = 0, 0.0
            for p in range(min(K, len(row))):
                if int(row[p]) in gts:
                    hits += 1
                    acc += hits / (p + 1)
            ap[q, j] = acc / min(len(gts), K)
            rec[q, j] = float(int(tgt_idx[q]) in set(int(i) for i in row[:K]))
    out = {f"circo_map_at{K}": 100.0 * float(ap[:, j].mean()) for j, K in enumerate(KS)}
    out.update({f"circo_recall_at{K}": 100.0 * float(rec[:, j].mean()) for j, K in enumerate(KS)})
    return out, ap


def _padded(gt_lists):
    G = max(len(g) for g in gt_lists)
    return np.array([list(g) + [-1] * (G - len(g)) for g in gt_lists], dtype=np.int64)


# ---- dataset ------------------------------------------------------------------------------------------------------------------
def describe(image):
    return [image.mode, *image.size]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return CT.build_circo_tree(tmp_path_factory.mktemp("circo") / "CIRCO")


def test_tree_has_the_cases_the_tests_rely_on():
    ids, val, test = CT.annotations()
    assert len(ids) == CT.N_IMG == len(set(ids)) and ids != sorted(ids) and max(ids) - min(ids) > 10 * len(ids)
    assert len(val[0]["gt_img_ids"]) == 1 and len(val[1]["gt_img_ids"]) == 23 == CT.MAX_GTS
    assert any(a["gt_img_ids"][0] != a["target_img_id"] for a in val)
    assert any(len(set(a["gt_img_ids"])) < len(a["gt_img_ids"]) for a in val)
    assert all(a["target_img_id"] in a["gt_img_ids"] and a["reference_img_id"] not in a["gt_img_ids"] for a in val)
    assert len(test) == len(val) == CT.N_QUERY and "target_img_id" not in test[0]


def test_dataset_equals_the_reference_class_field_by_field(tree, golden_dir):
    from sprc_amd.data_utils import CIRCODataset
    golden = json.loads((golden_dir / "circo_items.json").read_text())
    assert set(golden) == {"val/classic", "val/relative", "test/classic", "test/relative"}
    for key, want in golden.items():
        split, mode = key.split("/")
        ds = CIRCODataset(tree["root"], split, mode, describe)
        assert len(ds) == want["len"] and ds.max_num_gts == want["max_num_gts"] == 23
        items = [ds[i] for i in range(len(ds))]
        assert [sorted(i) for i in items] == [sorted(i) for i in want["items"]]          # the same keys, `reference_imd_id` included
        for got, exp in zip(items, want["items"]):
            for field, value in exp.items():
                assert got[field] == value, (key, field)
        assert ds.names == [str(i) for i in tree["ids"]]
        if split == "val":
            assert [ds.get_target_img_ids(i) for i in range(len(ds.annotations))] == want["target_img_ids"]
    assert items and isinstance(items[0]["query_id"], str)


def test_dataset_argument_errors_and_metadata_accessor(tree):
    from sprc_amd.data_utils import CIRCODataset
    from sprc_amd.dist_eval import gallery_names
    with pytest.raises(ValueError, match=r"split should be in \['test', 'val'\]"):
        CIRCODataset(tree["root"], "train", "classic", describe)
    with pytest.raises(ValueError, match=r"mode should be in \['relative', 'classic'\]"):
        CIRCODataset(tree["root"], "val", "both", describe)
    opened = []

    def counting(image):
        opened.append(image)
        return describe(image)

    ds = CIRCODataset(tree["root"], "val", "relative", counting)
    for i in range(len(ds)):
        meta, item = ds.query(i), None
        assert not opened, "query() must not open an image file"
        item = ds[i]
        assert len(opened) == 2 and {k: v for k, v in item.items() if k not in ("reference_img", "target_img")} == meta
        opened.clear()
    assert "target_img_id" not in CIRCODataset(tree["root"], "test", "relative", describe).query(0)
    assert gallery_names(CIRCODataset(tree["root"], "val", "classic", describe)) == [str(i) for i in tree["ids"]]


def test_harness_index_mapping_removes_duplicates_and_refuses_bad_queries(tree):
    from sprc_amd.data_utils import CIRCODataset
    from sprc_amd.harness import circo_indices, circo_reference_ids
    ds = CIRCODataset(tree["root"], "val", "relative", describe)
    names = [str(i) for i in tree["ids"]]
    q = [ds.query(i) for i in range(len(ds))]
    gt_idx, tgt_idx = circo_indices(names, [x["target_img_id"] for x in q], [x["gt_img_ids"] for x in q])
    assert gt_idx.shape == (10, 23) and (gt_idx[1] >= 0).all() and (gt_idx[0] >= 0).sum() == 1
    for row, a in zip(gt_idx, tree["val"]):
        assert [names[i] for i in row if i >= 0] == list(dict.fromkeys(str(g) for g in a["gt_img_ids"]))
    assert [names[i] for i in tgt_idx] == [str(a["target_img_id"]) for a in tree["val"]]
    assert circo_reference_ids(ds) == [str(a["reference_img_id"]) for a in tree["val"]]
    with pytest.raises(ValueError, match="no ground truth"):
        circo_indices(names, [names[0]], [["", ""]])
    with pytest.raises(ValueError, match="not in the gallery"):
        circo_indices(names, [names[0]], [[names[0], "12"]])
    with pytest.raises(ValueError, match="not in the gallery"):
        circo_indices(names, ["12"], [[names[0]]])


# ---- host metric of the sharded path --------------------------------------------------------------------------------------------
def _random_problem(seed, nq=40, N=173, quantise=False):
    rng = np.random.default_rng(seed)
    sim = rng.uniform(-1, 1, size=(nq, N)).astype(np.float32)
    if quantise:
        sim = (np.round(sim * 64) / 64).astype(np.float32)                    # rows full of ties: the index decides
    gt_lists = [rng.choice(N, size=int(rng.integers(1, 24)), replace=False).tolist() for _ in range(nq)]
    tgt = np.array([g[int(rng.integers(0, len(g)))] if q % 4 else int(rng.integers(0, N)) for q, g in enumerate(gt_lists)])
    return sim, gt_lists, tgt


@pytest.mark.parametrize("quantise", [False, True], ids=["random", "ties"])
def test_metrics_from_topk_equal_brute_force(quantise):
    from sprc_amd.dist_eval import circo_metrics_from_topk
    for seed in range(3):
        sim, gt_lists, tgt = _random_problem(seed, quantise=quantise)
        if quantise:
            assert max(len(np.unique(r)) for r in sim) <= 129 < sim.shape[1]
        order = np.argsort(np.float32(1.0) - sim, axis=1, kind="stable")
        want, _ = brute_circo(sim, gt_lists, tgt)
        assert circo_metrics_from_topk(order[:, :50], _padded(gt_lists), tgt) == want
    # a gallery smaller than 50: the unused slots of the top-k are -1
    sim, gt_lists, tgt = _random_problem(9, nq=12, N=30, quantise=quantise)
    gt_lists = [[g % 30 for g in dict.fromkeys(x % 30 for x in gl)] for gl in gt_lists]
    order = np.argsort(np.float32(1.0) - sim, axis=1, kind="stable")
    top = np.concatenate([order, np.full((12, 20), -1)], axis=1)
    assert circo_metrics_from_topk(top, _padded(gt_lists), tgt % 30) == brute_circo(sim, gt_lists, tgt % 30)[0]
    with pytest.raises(AssertionError):
        circo_metrics_from_topk(order[:, :10], _padded(gt_lists), tgt % 30)              # 10 of 30: not enough for K = 25


def test_hand_worked_average_precision():
    """ranks {0, 2, 5}, G = 3: AP@5 = (1/1 + 2/3) / 3, AP@10 = (1/1 + 2/3 + 3/6) / 3."""
    from sprc_amd.dist_eval import circo_metrics_from_topk
    top = np.arange(60)[None, :50]
    out = circo_metrics_from_topk(top, np.array([[5, 0, 2, -1]]), np.array([2]))
    assert out["circo_map_at5"] == pytest.approx(100 * (1 / 1 + 2 / 3) / 3, abs=1e-12)
    assert out["circo_map_at10"] == pytest.approx(100 * (1 / 1 + 2 / 3 + 3 / 6) / 3, abs=1e-12)
    assert out["circo_map_at25"] == out["circo_map_at50"] == out["circo_map_at10"]
    assert [out[f"circo_recall_at{k}"] for k in KS] == [100.0] * 4
    # more ground truths than K: the denominator is K
    out = circo_metrics_from_topk(top, np.array([[0, 1, 2, 3, 4, 5, 6, 40]]), np.array([40]))
    assert out["circo_map_at5"] == pytest.approx(100.0, abs=1e-12) and out["circo_map_at10"] == pytest.approx(100 * 7 / 8, abs=1e-12)
    assert [out[f"circo_recall_at{k}"] for k in KS] == [0.0, 0.0, 0.0, 100.0]


# ---- sharded evaluation on gloo ranks ---------------------------------------------------------------------------------------------
class CircoRelative(torch.utils.data.Dataset):
    """CIRCO val items (without images) over tests/_dist_case.py: ground truths = the subset members but the reference."""

    def __init__(self, case, test=False):
        self.case, self.test = case, test

    def __len__(self):
        return len(self.case["ref"])

    def __getitem__(self, i):
        c = self.case
        item = {"reference_imd_id": f"img-{c['ref'][i]:05d}", "relative_caption": f"q{i}", "shared_concept": "", "query_id": str(400 + i)}
        if not self.test:
            gts = [f"img-{g:05d}" for g in c["groups"][i] if g != c["ref"][i]]
            item.update(target_img_id=f"img-{c['tgt'][i]:05d}", gt_img_ids=gts + [""] * (23 - len(gts)))
        return item


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from sprc_amd import dist_eval as DE
    from test_dist_cpu import _cpu_sim, _cpu_topk
    from test_dist_eval_cpu import _setup
    cfg, sd, case, model = _setup()
    gallery = DC.Gallery(case["images"])
    local = {}

    def sim_fn(fusion, feats):
        s = _cpu_sim(fusion, feats)
        local["sim"] = s.clone()
        return s

    kw = dict(fuse_fn=model.fuse_captions, sim_fn=sim_fn, topk_fn=_cpu_topk, num_workers=0, gallery_batch_size=8)
    metrics = DE.compute_circo_val_metrics_sharded(CircoRelative(case), gallery, model, DC.TXT, **kw)
    top = DE.generate_circo_test_dicts_sharded(CircoRelative(case, test=True), gallery, model, DC.TXT, **kw)
    out[rank] = dict(metrics=metrics, top=top, sim=local["sim"].numpy())
    dist.barrier()
    dist.destroy_process_group()


def _check(world):
    from test_dist_eval_cpu import _free_port
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
        res = {r: dict(out[r]) for r in range(world)}
    case = DC.build(0)
    names = [f"img-{i:05d}" for i in case["keep"]]
    for r in range(world):
        assert res[r]["metrics"] == res[0]["metrics"] and res[r]["top"] == res[0]["top"]
    # the shards' score blocks tile the [nq, N] matrix: the single-process evaluation of it gives the same numbers, exactly
    sim = np.concatenate([res[r]["sim"] for r in range(world)], axis=1)
    assert sim.shape == (DC.NQ, len(names)) and len(names) > 50
    ref, tgt, grp = (DC.to_kept_index(case, case[k]) for k in ("ref", "tgt", "groups"))
    gt_lists = [[int(g) for g in grp[q] if g != ref[q]] for q in range(DC.NQ)]
    want, _ = brute_circo(sim, gt_lists, tgt)
    assert res[0]["metrics"] == want
    assert set(want) == {f"circo_{m}_at{k}" for m in ("map", "recall") for k in KS}
    order = np.argsort(np.float32(1.0) - sim, axis=1, kind="stable")
    assert res[0]["top"] == {str(400 + q): [names[i] for i in order[q, :50]] for q in range(DC.NQ)}


def test_sharded_circo_world2():
    _check(2)


def test_sharded_circo_world3_ragged():
    _check(3)


def test_unknown_dataset_message_names_all_three():
    from sprc_amd import blip_validate as bv
    with pytest.raises(ValueError, match="CIRR.*FashionIQ.*CIRCO"):
        bv.main(["--dataset", "imagenet"])


def test_feature_store_keeps_raw_rows_of_named_images_only(tmp_path):
    """sprc_amd/index.py with `raw_names`: what a CIRCO store holds -- raw embeddings of the queries' reference images, by name."""
    from sprc_amd.harness import RawStore
    from sprc_amd.index import load_index, save_index
    g = torch.Generator().manual_seed(0)
    feats = torch.nn.functional.normalize(torch.randn((9, 32, 16), generator=g), dim=-1)
    names = [str(7 * i % 9 + 100) for i in range(9)]
    raw = torch.randn((3, 5, 8), generator=g)
    kept = [names[6], names[0], names[4]]
    save_index(tmp_path / "s.safetensors", feats, names, raw=raw, raw_names=kept)
    (f2, r2), n2, meta = load_index(tmp_path / "s.safetensors")
    assert isinstance(r2, RawStore) and len(r2) == 9 and r2.kept == 3 and n2 == names and torch.equal(f2, feats) and "raw_names" not in meta
    assert torch.equal(r2[6], raw[0]) and torch.equal(r2[0], raw[1]) and torch.equal(r2[4], raw[2]) and r2[1] is None
    assert [r is not None for r in dict(zip(n2, r2)).values()] == [i in (0, 4, 6) for i in range(9)]
    with pytest.raises(ValueError, match="one entry per"):
        save_index(tmp_path / "bad.safetensors", feats, names, raw=raw, raw_names=kept[:2])
    with pytest.raises(ValueError, match="raw_names"):
        save_index(tmp_path / "bad.safetensors", feats, names, raw=raw, raw_names=["nope", names[0], names[1]])


def test_datasets_keep_the_root_they_were_built_over(tmp_path, monkeypatch):
    """Items are produced in loader workers; a worker started from a fork server sees the data root of the SERVER's environment.
    A dataset must therefore read from the directory it was constructed over, whatever `base_path` is where the item is made."""
    import pickle
    from PIL import Image
    import sprc_amd.data_utils as du
    cirr, fiq = tmp_path / "cirr_dataset", tmp_path / "fashionIQ_dataset"
    for d in (cirr / "cirr" / "captions", cirr / "cirr" / "image_splits", cirr / "img", fiq / "captions", fiq / "image_splits", fiq / "images"):
        d.mkdir(parents=True)
    Image.fromarray(CT.synth_image(40, 30, 1)).save(cirr / "img" / "a.png")
    Image.fromarray(CT.synth_image(30, 40, 2)).save(fiq / "images" / "b.png")
    (cirr / "cirr" / "captions" / "cap.rc2.val.json").write_text("[]")
    (cirr / "cirr" / "image_splits" / "split.rc2.val.json").write_text(json.dumps({"a": "img/a.png"}))
    (fiq / "captions" / "cap.dress.val.json").write_text("[]")
    (fiq / "image_splits" / "split.dress.val.json").write_text(json.dumps(["b"]))
    monkeypatch.setattr(du, "base_path", tmp_path)
    c = du.CIRRDataset("val", "classic", describe)
    f = du.FashionIQDataset("val", ["dress"], "classic", describe)
    monkeypatch.setattr(du, "base_path", tmp_path / "elsewhere")
    assert pickle.loads(pickle.dumps(c))[0] == ("a", ["RGB", 40, 30]) and pickle.loads(pickle.dumps(f))[0] == ("b", ["RGB", 30, 40])
