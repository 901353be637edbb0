"""A small, deterministic CIRCO tree on disk (shared by tests/test_circo_cpu.py, tests/test_circo_gpu.py and
tools/gen_circo_golden.py): the benchmark's directory layout (COCO2017_unlabeled/annotations/image_info_unlabeled2017.json,
COCO2017_unlabeled/unlabeled2017/<file_name>, annotations/{val,test}.json) with

* COCO-style image ids that are neither contiguous nor sorted (an id / index mix-up cannot pass),
* images of assorted sizes, one of them a grayscale file,
* a query with a single ground truth and one with 23 (the benchmark's maximum: every image but its reference),
* targets that are not the first entry of their ground-truth list,
* one ground-truth list that names an image twice.

The reference image and the caption of query j come from QUERY_SEEDS[j] alone.  Those ten seeds were chosen on the CPU,
with the fp32 oracle alone (tests/test_circo_gpu.py states the procedure and asserts its outcome): every query's 24 oracle
scores lie more than 1e-4 apart, so the fp32 engine (documented to hold 6e-6) must reproduce the oracle's order exactly.
"""
import json
from pathlib import Path

import numpy as np
from PIL import Image

N_IMG, N_QUERY, MAX_GTS = 24, 10, 23
SIZES = [(320, 240), (200, 400), (224, 224), (420, 130), (97, 301), (233, 233), (260, 190)]
GRAY = 5                                    # position (file order) of the grayscale image
WORDS = ["make", "the", "dog", "bigger", "remove", "person", "add", "a", "red", "hat", "and", "two", "cats", "instead", "of", "one",
         "brighter", "background", "is", "more", "colour", "##ful", "##s", "##er", "left", "right"]
CONCEPTS = ["a dog", "two cats", "a person with a hat", "the background"]
QUERY_SEEDS = [8, 15, 25, 62, 92, 117, 123, 134, 162, 182]


def synth_image(w: int, h: int, seed: int) -> np.ndarray:
    """smooth structure + noise, uint8 RGB [h, w, 3]"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([127 + 90 * np.sin(xx / (6.0 + c + seed % 5) + yy / (12.0 - c)) + rng.normal(0, 25, (h, w)) for c in range(3)], axis=-1)
    return np.clip(img, 0, 255).astype(np.uint8)


def query_of(seed: int, ids):
    """-> (reference id, caption) of the query drawn from `seed`."""
    rng = np.random.default_rng(7000 + seed)
    ref = int(ids[int(rng.integers(0, len(ids)))])
    cap = " ".join(rng.choice(WORDS[:20], size=int(rng.integers(3, 10))).tolist()).capitalize() + "."
    return ref, cap


def annotations(query_seeds=QUERY_SEEDS):
    """-> (ids in file order, val annotations, test annotations); no file is touched."""
    rng = np.random.default_rng(2017)
    ids = [int(i) for i in rng.choice(np.arange(139, 581930), size=N_IMG, replace=False)]       # unsorted, far from contiguous
    assert ids != sorted(ids)
    val = []
    for j, seed in enumerate(query_seeds):
        ref, cap = query_of(seed, ids)
        others = [i for i in ids if i != ref]
        n_gt = {0: 1, 1: MAX_GTS}.get(j, int(rng.integers(2, 9)))
        gts = [int(g) for g in rng.choice(others, size=n_gt, replace=False)]
        tgt = gts[0] if n_gt == 1 else gts[int(rng.integers(1, n_gt))]                          # not first wherever there is a choice
        if j == 2:
            gts.append(gts[1])                                                                   # a duplicated ground-truth id
        val.append({"id": 300 + 7 * j, "reference_img_id": ref, "target_img_id": tgt, "gt_img_ids": gts, "relative_caption": cap,
                    "shared_concept": CONCEPTS[j % len(CONCEPTS)]})
    test = [{"id": 9000 + 3 * j, "reference_img_id": a["reference_img_id"], "relative_caption": a["relative_caption"],
             "shared_concept": a["shared_concept"]} for j, a in enumerate(reversed(val))]
    return ids, val, test


def build_circo_tree(root, query_seeds=QUERY_SEEDS) -> dict:
    """Write the tree under `root` -> dict(root, ids, arrays {str(id): uint8 RGB array as the transform sees it}, val, test)."""
    root = Path(root)
    coco = root / "COCO2017_unlabeled"
    (coco / "annotations").mkdir(parents=True, exist_ok=True)
    (coco / "unlabeled2017").mkdir(parents=True, exist_ok=True)
    (root / "annotations").mkdir(parents=True, exist_ok=True)
    ids, val, test = annotations(query_seeds)
    info, arrays = [], {}
    for k, i in enumerate(ids):
        w, h = SIZES[k % len(SIZES)]
        arr = synth_image(w, h, 500 + k)
        name = f"{i:012d}.png"
        if k == GRAY:
            Image.fromarray(arr[:, :, 0], mode="L").save(coco / "unlabeled2017" / name)
            arr = np.stack([arr[:, :, 0]] * 3, axis=-1)
        else:
            Image.fromarray(arr).save(coco / "unlabeled2017" / name)
        info.append({"id": i, "file_name": name, "width": w, "height": h})
        arrays[str(i)] = arr
    (coco / "annotations" / "image_info_unlabeled2017.json").write_text(json.dumps({"images": info}))
    (root / "annotations" / "val.json").write_text(json.dumps(val))
    (root / "annotations" / "test.json").write_text(json.dumps(test))
    return dict(root=root, ids=ids, arrays=arrays, val=val, test=test)
