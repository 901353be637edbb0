#!/usr/bin/env python3
"""Record what the reference's CIRCODataset (src/data_utils.py:289-426) yields over the synthetic CIRCO tree of
tests/_circo_tree.py -> tests/golden/circo_items.json (data only: lengths, ids, captions, shared concepts, padded
ground-truth lists, and -- in place of pixels -- the [mode, width, height] of every image the class opened).

Needs the reference checkout (oracle/ref_import.py); tests/test_circo_cpu.py compares sprc_amd.data_utils.CIRCODataset
with the recorded file and needs only the file.   python tools/gen_circo_golden.py
"""
import json
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

from _circo_tree import build_circo_tree  # noqa: E402
from oracle import ref_import  # noqa: E402


def describe(image):
    """stands in for the image transform: what was opened, not its pixels"""
    return [image.mode, *image.size]


def main():
    ref_import.import_harness()                       # puts the reference's src/ on the path, with the import shims
    import data_utils as ref_du
    out = {}
    with tempfile.TemporaryDirectory() as d:
        tree = build_circo_tree(Path(d) / "CIRCO")
        for split in ("val", "test"):
            for mode in ("classic", "relative"):
                ds = ref_du.CIRCODataset(tree["root"], split, mode, describe)
                rec = {"len": len(ds), "items": [ds[i] for i in range(len(ds))], "max_num_gts": ds.max_num_gts}
                if split == "val":
                    rec["target_img_ids"] = [ds.get_target_img_ids(i) for i in range(len(ds.annotations))]
                out[f"{split}/{mode}"] = rec
    path = ROOT / "tests" / "golden" / "circo_items.json"
    path.write_text(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
