#!/usr/bin/env python3
"""Record what the reference's fine-tuning script does on the host side -> tests/golden/ (data only: inputs and recorded outputs).

  fiq_randomized_captions.json   64 caption pairs (some with leading / trailing '.?, ' characters) and what the UNMODIFIED
                                 utils.generate_randomized_fiq_caption (src/utils.py:117-138) returns for them under
                                 random.seed(0..3)
  finetune_arg_defaults.json     the defaults of the arguments src/blip_fine_tune_2.py:370-391 declares (its parser lives under
                                 `if __name__ == '__main__'`, so the add_argument calls are read from the syntax tree)

Needs the reference checkout (oracle/ref_import.py); tests/test_finetune_host.py needs only the files.
    python tools/gen_finetune_golden.py
"""
import ast
import json
import random
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import ref_import  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
WORDS = ["is", "more", "red", "has", "longer", "sleeves", "shorter", "and", "darker", "with", "a", "floral", "print", "less", "formal",
         "blue", "striped", "collar", "no", "buttons", "lighter", "looser", "fit", "v-neck", "graphic", "plain"]
EDGES = ["", ".", "?", ",", " ", ". ", " .", "?, ", ",. ?"]


def caption_pairs(n: int = 64, seed: int = 5):
    rng = random.Random(seed)
    flat = []
    for i in range(2 * n):
        body = " ".join(rng.choice(WORDS) for _ in range(rng.randint(1, 6)))
        if i % 3 == 0:
            body = body.capitalize()
        if i % 11 == 0:
            body = body.upper()
        flat.append(rng.choice(EDGES) + body + rng.choice(EDGES))
    return flat


def argument_defaults():
    tree = ast.parse((ref_import.SRC / "blip_fine_tune_2.py").read_text())
    out = {}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            flag = ast.literal_eval(node.args[0])
            kw = {k.arg: k.value for k in node.keywords}
            if "default" in kw:
                default = ast.literal_eval(kw["default"])
            elif "action" in kw and ast.literal_eval(kw["action"]) == "store_true":
                default = False
            else:
                default = None
            out[flag] = {"default": default, "required": bool("required" in kw and ast.literal_eval(kw["required"]))}
    return out


def main():
    ref_import.import_harness()
    import utils as ref_utils                     # the reference's src/utils.py
    flat = caption_pairs()
    runs = {}
    for seed in range(4):
        random.seed(seed)
        runs[str(seed)] = ref_utils.generate_randomized_fiq_caption(list(flat))
    assert len({tuple(v) for v in runs.values()}) == 4
    (GOLDEN / "fiq_randomized_captions.json").write_text(json.dumps({"flattened_captions": flat, "by_seed": runs}, indent=1) + "\n")
    args = argument_defaults()
    assert "--dataset" in args and len(args) >= 17
    (GOLDEN / "finetune_arg_defaults.json").write_text(json.dumps(args, indent=1, sort_keys=True) + "\n")
    print("wrote", GOLDEN / "fiq_randomized_captions.json", GOLDEN / "finetune_arg_defaults.json")


if __name__ == "__main__":
    main()
