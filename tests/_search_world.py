"""Shared pieces of the per-query-filter search tests (tests/test_search_admit_gpu.py): the exact-data case, admit words from per-query
sets, and the small synthetic world (checkpoint, vocabulary, PNG files, store) that `Searcher` and the command line run on."""
import os
import sys
from pathlib import Path

import numpy as np
import torch

_EXACT = {}


def exact_case(N):
    """(queries [32,256] fp32, gallery [N,32,256] fp32) holding integers in [-8, 8] x 2^-6 -- every product a multiple of 2^-12 and every
    256-term sum below 4, so fp32 accumulation is exact in any order -- and a function rows -> float64 scores [32, len(rows)], evaluated
    at the listed images only, in chunks."""
    if N not in _EXACT:
        rng = np.random.default_rng(2000 + N)
        q = rng.integers(-8, 9, size=(32, 256)).astype(np.float64) / 64.0
        f = rng.integers(-8, 9, size=(N, 32, 256), dtype=np.int8)
        _EXACT[N] = (torch.from_numpy(q.astype(np.float32)), torch.from_numpy(f), q, f)
    q32, f8, q, f = _EXACT[N]

    def ref(rows):
        rows = np.asarray(rows)
        out = np.empty((32, len(rows)))
        for s in range(0, len(rows), 2048):
            fr = f[rows[s:s + 2048]].astype(np.float64) / 64.0
            out[:, s:s + len(fr)] = (fr.reshape(-1, 256) @ q.T).reshape(len(fr), 32, 32).max(axis=1).T
        return out
    return q32, f8, ref


def admit_words(member):
    """member: bool [nq, M] (query q admits list position m) -> int32 tensor [ceil(nq / 32), M] of uint32 bit patterns."""
    member = np.asarray(member, dtype=bool)
    nq, M = member.shape
    words = np.zeros((-(-nq // 32), M), dtype=np.uint32)
    for q in range(nq):
        words[q // 32] |= member[q].astype(np.uint32) << np.uint32(q % 32)
    return torch.from_numpy(words.view(np.int32).copy())


def admitted(words, nq):
    """The inverse: uint32 words [M] of one block -> bool [nq, M]."""
    words = np.asarray(words, dtype=np.uint32)
    return ((words[None, :] >> np.arange(nq, dtype=np.uint32)[:, None]) & 1).astype(bool)


N_IMG, DEPTH = 14, 1
WORDS = ["make", "the", "dog", "bigger", "remove", "person", "add", "a", "red", "hat", "and", "two", "cats", "instead", "of", "one",
         "brighter", "background", "is", "more", "colour", "##ful", "##s", "##er", "left", "right"]
CAPTIONS = ["Make the dog bigger and add a red hat.", "Remove the person and add two cats.", "The background is brighter.",
            "Two cats instead of one dog."]


def make_world(root: Path):
    """14 PNG files of assorted sizes, a synthetic vocabulary, a depth-1 checkpoint and the fp16 store `search build` writes for them ->
    (dict, the value SPRC_BERT_VOCAB had before).  Sets SPRC_BERT_VOCAB: the caller restores it."""
    from PIL import Image
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    from gen_preprocess_golden import synth_image
    from sprc_amd import search, synth
    from sprc_amd.config import get_config
    (root / "images" / "more").mkdir(parents=True)
    sizes = [(500, 375), (300, 600), (224, 224), (640, 200), (97, 301), (333, 333), (260, 190)]
    names, files = [], {}
    for i in range(N_IMG):
        w, h = sizes[i % len(sizes)]
        arr = synth_image(w, h, 170 + i)
        name = f"item-{i:03d}"
        files[name] = root / "images" / ("more" if i % 5 == 0 else ".") / f"{name}.png"
        if i == 4:                                            # one grayscale file
            Image.fromarray(arr[:, :, 0], mode="L").save(files[name])
        else:
            Image.fromarray(arr).save(files[name])
        names.append(name)
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + [".", ","]
    vocab += [f"tok{i}" for i in range(30522 - len(vocab))]
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    cfg = get_config("pretrain", vit_depth=DEPTH)
    torch.save({"Blip2QformerCirAlignPrompt": synth.make_state_dict(cfg, seed=29), "epoch": 0}, root / "ckpt.pt")
    before = os.environ.get("SPRC_BERT_VOCAB")
    os.environ["SPRC_BERT_VOCAB"] = str(root / "vocab.txt")
    base = ["--model-path", str(root / "ckpt.pt"), "--dtype", "fp16", "--vit-depth", str(DEPTH)]
    built = search.main(["build", "--images", str(root / "images"), "--out", str(root / "store.safetensors"), "--feats-dtype", "fp16"] + base)
    assert built["images"] == N_IMG
    return dict(root=root, names=names, files=files, base=base, store=str(root / "store.safetensors")), before
