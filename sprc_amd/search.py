#!/usr/bin/env python3
"""Index search: one reference image + one caption -> the best-matching gallery names of a stored index.

    python -m sprc_amd.search build --images DIR --model-path X --out STORE [--backbone B --dtype fp16 --feats-dtype fp16
                                    --keep-raw all|none --gpu-preprocess]
    python -m sprc_amd.search query --index STORE --model-path X (--reference NAME | --reference-image FILE) --caption "..."
                                    [-k 10] [--json]

    s = Searcher(model, "gallery.safetensors")
    s.search(["dog-017", "/tmp/photo.jpg"], ["the same dog on a beach", "make it night"], k=10)

No reference counterpart: the reference ranks inside its evaluation loops only (validate_blip.py:253-254).  The pieces are the
evaluation path's own -- caption processor, tokenizer, `model.fuse` -- followed by `engine.search_topk` on the store's 16-bit
`feats`: the streaming score kernel (csrc/search.hip) and the two-level top-k.  The gallery is uploaded once, when the Searcher
is made; a search does no per-gallery-item work on the host.
"""
from __future__ import annotations

import json
import os
import time
from argparse import ArgumentParser
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import engine as E

# Queries per search above which the scores come from the GEMM (E.sim_max) instead of the streaming kernel; the top-k is
# two-level either way.  profiles/search_bench.txt, lines "N = 123403" / "N = 1000000": the stream kernel walks the gallery once
# per 32 queries, so up to nq = 32 arm (a) is ahead of or level with both GEMM arms (nq = 32: 595 us vs (b2) 588 us at 123 403
# images, 3836 vs 4096 us at 10^6), and from nq = 64 (two walks) the GEMM arms win ((a) 1088 us vs (b2) 732 us, 7345 vs 4583 us).
STREAM_MAX_QUERIES = 32

_RANK_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
MODEL_NAME = "blip2_cir_align_prompt"            # the command line's model class (stage 1; `--rerank` is out of scope here)


class _RawRows:
    """name -> raw ViT embeddings of a stored gallery image (a stacked tensor or a `harness.RawStore`), None when not kept:
    the mapping `harness._stack_refs` takes."""

    def __init__(self, raw, row_of: Dict[str, int]):
        self.raw, self.row_of = raw, row_of

    def get(self, name):
        i = self.row_of.get(name)
        return None if i is None or self.raw is None else self.raw[i]

    def __getitem__(self, name):
        return self.raw[self.row_of[name]]


class Searcher:
    def __init__(self, model, index_path, rank_dtype: Optional[str] = None, preprocess=None):
        """rank_dtype None: the store's dtype; an fp32 store is rounded once, here, to the engine's 16-bit dtype (fp16 for the
        fp32 engine).  preprocess: the transform of image FILES given as references -- the one the gallery was built with
        (default `targetpad_transform(1.25, 224)`; `GpuTargetPad` is bit-identical)."""
        from .blip_validate import model_fingerprint
        from .index import load_index
        self.model = model
        dev = model.device
        (feats, raw), names, meta = load_index(index_path, device=dev, keep_feats_dtype=True)
        fp = model_fingerprint(model)
        if meta.get("checkpoint_sha256") != fp:
            raise ValueError(f"{index_path}: written by another checkpoint ({str(meta.get('checkpoint_sha256', '?'))[:16]}, this model is "
                             f"{fp[:16]}): features of one checkpoint are never ranked with the queries of another")
        if rank_dtype is None:
            eng = model.engine()
            rdt = feats.dtype if feats.dtype != torch.float32 else (eng.tdt if eng.is16 else torch.float16)
        elif rank_dtype in _RANK_DTYPES:
            rdt = _RANK_DTYPES[rank_dtype]
        else:
            raise ValueError(f"rank_dtype {rank_dtype!r}: the index search ranks on fp16 or bf16 operands")
        self.rank_dtype = rdt
        self.feats = feats.to(rdt).contiguous()
        self.names: List[str] = list(names)
        self.meta = meta
        self._raw = _RawRows(raw, {n: i for i, n in enumerate(self.names)})
        if preprocess is None:
            from .data_utils import targetpad_transform
            preprocess = targetpad_transform(1.25, 224)
        self.preprocess = preprocess
        from .processors import BlipCaptionProcessor
        self.txt_processors = {"eval": BlipCaptionProcessor()}

    # ---- references ---------------------------------------------------------------------------------
    def _encode_images(self, images: torch.Tensor) -> torch.Tensor:
        return self.model.extract_target_features(images.to(self.model.device, torch.float32))[1]

    def reference_embeds(self, reference: Sequence) -> torch.Tensor:
        """A list mixing gallery names (embeddings from the store's `raw`), transformed image tensors [B,3,224,224] / [3,224,224]
        and image files (decoded, transformed, encoded) -> raw ViT embeddings [B, tokens, D] fp32 in list order."""
        from .harness import _stack_refs
        if isinstance(reference, (str, Path, torch.Tensor)):
            reference = [reference]
        dev = self.model.device
        out = []
        for r in reference:
            if isinstance(r, torch.Tensor):
                out.append(self._encode_images(r if r.dim() == 4 else r.unsqueeze(0)).float())
            elif isinstance(r, str) and r in self._raw.row_of:
                out.append(_stack_refs(self._raw, [r]).to(dev))
            elif isinstance(r, (str, Path)) and os.path.isfile(r):
                from PIL import Image
                out.append(self._encode_images(self.preprocess(Image.open(r)).unsqueeze(0)).float())
            else:
                raise KeyError(f"reference {r!r} is neither a gallery name of this index nor an image file")
        return out[0] if len(out) == 1 else torch.cat(out)

    # ---- search -------------------------------------------------------------------------------------
    @torch.no_grad()
    def search_ids(self, reference, input_ids: torch.Tensor, attention_mask: torch.Tensor, k: int,
                   timings: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [B,k] fp32, gallery rows [B,k] int32; -inf / -1 beyond the gallery's size).  timings: a dict that receives
        the milliseconds of the three phases (reference embeddings, fuse, rank), each ended by a device synchronisation."""
        dev = self.model.device

        def lap(key, t0):
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings[key] = (time.perf_counter() - t0) * 1e3
            return time.perf_counter()

        t = time.perf_counter()
        with torch.cuda.device(dev):
            ref = self.reference_embeds(reference)
            if ref.shape[0] != input_ids.shape[0]:
                raise ValueError("one caption per reference image is required")
            t = lap("reference_ms", t)
            fusion = self.model.fuse(ref, input_ids.to(dev), attention_mask.to(dev))
            fusion = fusion.to(self.rank_dtype).contiguous()
            t = lap("fuse_ms", t)
            if fusion.shape[0] <= STREAM_MAX_QUERIES:
                vals, idx = E.search_topk(fusion, self.feats, k)
            else:
                sim = E.sim_max(fusion, self.feats, out=E.segmented_sim_buffer(fusion.shape[0], self.feats.shape[0], dev))
                vals, idx = E.topk_segmented(sim, k)
            lap("rank_ms", t)
        return vals, idx

    def search(self, reference, captions: Union[str, Sequence[str]], k: int = 10, timings: Optional[dict] = None) -> List[List[Tuple[str, float]]]:
        if isinstance(captions, str):
            captions = [captions]
        text = [self.txt_processors["eval"](c) for c in captions]
        tok = self.model.tokenizer(text, padding="max_length", truncation=True, max_length=self.model.max_txt_len, return_tensors="pt")
        vals, idx = self.search_ids(reference, tok.input_ids, tok.attention_mask, k, timings=timings)
        vals, idx = vals.cpu().tolist(), idx.cpu().tolist()
        return [[(self.names[i], float(v)) for v, i in zip(vr, ir) if i >= 0] for vr, ir in zip(vals, idx)]


# ---- command line ---------------------------------------------------------------------------------------
def _parser() -> ArgumentParser:
    p = ArgumentParser(prog="python -m sprc_amd.search")
    sub = p.add_subparsers(dest="command", required=True)

    def common(q):
        q.add_argument("--model-path", type=str, required=True)
        q.add_argument("--backbone", type=str, default="pretrain", help="pretrain for vit-g, pretrain_vitL for vit-l")
        q.add_argument("--dtype", default="fp16", choices=["bf16", "fp16", "fp32"], help="the engine's compute dtype")
        q.add_argument("--gpu-preprocess", action="store_true", help="pad / bicubic resize / crop / normalise on the GPU (bit-identical)")
        q.add_argument("--vit-depth", type=int, default=None, help="truncate the ViT to N blocks (smoke tests only)")

    b = sub.add_parser("build", help="encode a directory of images into a feature store")
    b.add_argument("--images", type=str, required=True, help="directory of image files; a file's stem is its gallery name")
    b.add_argument("--out", type=str, required=True)
    b.add_argument("--feats-dtype", default="fp16", choices=["fp16", "bf16", "fp32"], help="stored dtype of the ranking features")
    b.add_argument("--keep-raw", default="all", choices=["all", "none"], help="keep the ViT embeddings, so that gallery images can be references")
    common(b)
    q = sub.add_parser("query", help="rank a stored gallery for one reference image and one caption")
    q.add_argument("--index", type=str, required=True)
    ref = q.add_mutually_exclusive_group(required=True)
    ref.add_argument("--reference", type=str, help="a gallery name whose embeddings the store keeps")
    ref.add_argument("--reference-image", type=str, help="an image file")
    q.add_argument("--caption", type=str, required=True)
    q.add_argument("-k", type=int, default=10)
    q.add_argument("--json", action="store_true")
    common(q)
    return p


def build_index(a) -> dict:
    from .blip_validate import _load, _preprocess, _raw_store_dtype, model_fingerprint
    from .data_utils import ImageDirDataset
    from .harness import extract_index_blip_features
    from .index import save_index
    model, _ = _load(MODEL_NAME, a.backbone, a.model_path, a.dtype, a.vit_depth)
    preprocess, workers = _preprocess(a.gpu_preprocess, model.device)
    dataset = ImageDirDataset(a.images, preprocess)
    if len(dataset) == 0:
        raise SystemExit(f"search build: no image files under {a.images}")
    keep = a.keep_raw == "all"
    (feats, raw), names = extract_index_blip_features(dataset, model, num_workers=workers if len(dataset) >= 256 else 0, keep_raw=keep)
    if len(names) != len(dataset):
        raise SystemExit(f"search build: {len(dataset) - len(names)} of {len(dataset)} files could not be read")
    save_index(a.out, feats, names, raw=raw if keep else None, backbone=a.backbone, compute_dtype=a.dtype,
               checkpoint_sha256=model_fingerprint(model), raw_dtype=_raw_store_dtype(model),
               feats_dtype={"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.feats_dtype])
    out = {"index": str(a.out), "images": len(names), "feats_dtype": a.feats_dtype, "raw": keep}
    print(json.dumps(out))
    return out


def query_index(a) -> List[Tuple[str, float]]:
    from .blip_validate import _load, _preprocess
    model, _ = _load(MODEL_NAME, a.backbone, a.model_path, a.dtype, a.vit_depth)
    s = Searcher(model, a.index, preprocess=_preprocess(a.gpu_preprocess, model.device)[0])
    timings = {} if a.json else None
    hits = s.search([a.reference if a.reference is not None else Path(a.reference_image)], [a.caption], k=a.k, timings=timings)[0]
    if a.json:
        print(json.dumps({"caption": a.caption, "reference": a.reference or a.reference_image, "timings": timings,
                          "results": [{"rank": r + 1, "name": n, "score": v} for r, (n, v) in enumerate(hits)]}))
    else:
        for r, (n, v) in enumerate(hits):
            print(f"{r + 1:4d}  {n}  {v:.6f}")
    return hits


def main(argv=None):
    a = _parser().parse_args(argv)
    return build_index(a) if a.command == "build" else query_index(a)


if __name__ == "__main__":
    main()
