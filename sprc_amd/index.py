"""Feature store for an encoded gallery ("feature-store format for feats ... + names").

The reference re-encodes the whole gallery on every run (`src/utils.py:46-77` returns tensors that nobody persists;
`save_memory` only moves them to the CPU, `:67-69`).  A gallery is encoded once here and kept as ONE safetensors file:

    feats      [N, 32, 256]  fp32   unit-norm Q-Former query features (what `inference` ranks against); or fp16 / bf16
                                    (`feats_dtype`): exactly the bits a 16-bit rank dtype ranks on (`model.similarity` rounds
                                    before `sim_max`) and the operand `sprc_amd.search` streams, at half the bytes
    raw        [N, 257, D]   fp32, or the engine's 16-bit operand dtype (`raw_dtype`)
                                    optional: ViT embeddings of the images that can be *reference* images of a query
                                    (CIRR/FashionIQ take references from the gallery itself); omitted for pure galleries.
                                    fp16 / bf16: the format the engine rounds them to anyway when it reads them (the K|V
                                    projection operand of the fusion pass and of the rerank): half the bytes, the same bits
                                    downstream (the rounding is idempotent); load_index hands them back as fp32
                                    With `raw_names` (a gallery too large to keep every image's embeddings: CIRCO's 123 403
                                    images would be 178 GB) raw holds the rows of those images only, in that order, and
                                    load_index hands back a `harness.RawStore`
    metadata   names (JSON list, row order), raw_names (optional JSON list), backbone, dtype the features were computed in, format version,
               checkpoint_sha256 = fingerprint of the state dict that produced the features (blip_validate refuses a store
               written by another checkpoint)

Loading is a plain mmap + one host-to-device copy; ranking from a loaded store is bit-identical to ranking from the
tensors it was saved from (tests/test_host.py, tests/test_fullsize_gpu.py).

`append_index` / `remove_from_index` edit a stored gallery row-wise (the `add` / `remove` sub-commands of `sprc_amd.search`): the
file is read in its stored dtypes and rewritten by `save_index`, the format and its metadata keys unchanged.
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import torch

FORMAT = "sprc-index-1"
_DTYPE_NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def save_index(path, feats: torch.Tensor, names: Sequence[str], raw: Optional[torch.Tensor] = None, backbone: str = "",
               compute_dtype: str = "", checkpoint_sha256: str = "", raw_dtype: torch.dtype = torch.float32,
               raw_names: Optional[Sequence[str]] = None, feats_dtype: torch.dtype = torch.float32) -> None:
    """raw_names: `raw` holds the embeddings of these gallery images only (one row each, in this order).
    feats_dtype: float16 / bfloat16 store `feats` rounded to that dtype (recorded as `feats_dtype` in the metadata); the default
    writes the fp32 file this format has always had, without the key."""
    from safetensors.torch import save_file
    if feats.dim() != 3 or feats.shape[1] != 32:
        raise ValueError(f"feats must be [N,32,E], got {tuple(feats.shape)}")
    if len(names) != feats.shape[0] or (raw is not None and raw.shape[0] != (feats.shape[0] if raw_names is None else len(raw_names))):
        raise ValueError("names / raw must have one entry per gallery row")
    if raw_names is not None and (raw is None or not set(raw_names) <= set(names)):
        raise ValueError("raw_names must name gallery rows whose embeddings are given in `raw`")
    if len(set(names)) != len(names):
        raise ValueError("gallery names must be unique (they are the join key of the relative datasets)")
    if feats_dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"feats_dtype {feats_dtype}")
    tensors = {"feats": feats.detach().to(feats_dtype).to("cpu").contiguous()}         # rounded where the tensor lives, then copied
    if raw is not None:
        if raw_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError(f"raw_dtype {raw_dtype}")
        tensors["raw"] = raw.detach().to(raw_dtype).to("cpu").contiguous()          # rounded where the tensor lives (the GPU), then copied
    meta = {"format": FORMAT, "names": json.dumps(list(names)), "backbone": backbone, "compute_dtype": compute_dtype,
            "checkpoint_sha256": checkpoint_sha256}
    if raw_names is not None:
        meta["raw_names"] = json.dumps(list(raw_names))
    if feats_dtype != torch.float32:
        meta["feats_dtype"] = _DTYPE_NAMES[feats_dtype]
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    save_file(tensors, str(path), metadata=meta)


def load_index(path, device="cpu", with_raw: bool = True,
               keep_feats_dtype: bool = False) -> Tuple[Tuple[torch.Tensor, Optional[torch.Tensor]], List[str], dict]:
    """-> ((feats, raw or None), names, metadata) with the tensors on `device`: the `(index_features, index_names)` pair
    the reference's `compute_*_val_metrics` / `generate_*_predictions` take.  `feats` comes back as fp32 (a 16-bit store is
    upcast after the copy to `device`) unless keep_feats_dtype, which hands back the stored dtype; a file without `feats_dtype`
    in its metadata is an fp32 store."""
    from safetensors import safe_open
    with safe_open(str(path), framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a {FORMAT} file (format={meta.get('format')!r})")
        feats = f.get_tensor("feats")
        raw = f.get_tensor("raw") if with_raw and "raw" in f.keys() else None
    names = json.loads(meta["names"])
    if len(names) != feats.shape[0]:
        raise ValueError(f"{path}: {len(names)} names for {feats.shape[0]} rows")
    stored = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(meta.get("feats_dtype"), torch.float32)
    if feats.dtype != stored:
        raise ValueError(f"{path}: feats are {feats.dtype}, the metadata says {stored}")
    feats = feats.to(device)
    if not keep_feats_dtype:
        feats = feats.float()
    raw = raw.to(device).float() if raw is not None else None
    if raw is not None and "raw_names" in meta:
        from .harness import RawStore
        row_of = {n: i for i, n in enumerate(names)}
        raw = RawStore(len(names), {row_of[n]: raw[j] for j, n in enumerate(json.loads(meta["raw_names"]))})
    return (feats, raw), names, {k: v for k, v in meta.items() if k not in ("names", "raw_names")}


# ---- editing a stored gallery -----------------------------------------------------------------------------------------------------
def _read_store(path):
    """-> (feats, raw or None, names, raw_names or None, metadata) with the tensors in their STORED dtypes, on the CPU."""
    from safetensors import safe_open
    with safe_open(str(path), framework="pt", device="cpu") as f:
        meta = f.metadata() or {}
        if meta.get("format") != FORMAT:
            raise ValueError(f"{path}: not a {FORMAT} file (format={meta.get('format')!r})")
        feats = f.get_tensor("feats")
        raw = f.get_tensor("raw") if "raw" in f.keys() else None
    names = json.loads(meta["names"])
    if len(names) != feats.shape[0]:
        raise ValueError(f"{path}: {len(names)} names for {feats.shape[0]} rows")
    return feats, raw, names, (json.loads(meta["raw_names"]) if "raw_names" in meta else None), meta


def _write_store(path, feats, raw, names, raw_names, meta) -> None:
    """`save_index` with everything but the rows taken from the file's own metadata and tensors: dtypes, `raw_names`, backbone,
    compute dtype and fingerprint are kept, no key is added, so a store that loses or gains no row is rewritten unchanged."""
    save_index(path, feats, names, raw=raw, backbone=meta.get("backbone", ""), compute_dtype=meta.get("compute_dtype", ""),
               checkpoint_sha256=meta.get("checkpoint_sha256", ""), raw_dtype=raw.dtype if raw is not None else torch.float32,
               raw_names=raw_names, feats_dtype=feats.dtype)


def _same_checkpoint(path, meta, checkpoint_sha256) -> None:
    if checkpoint_sha256 is not None and meta.get("checkpoint_sha256") != checkpoint_sha256:
        raise ValueError(f"{path}: written by another checkpoint ({str(meta.get('checkpoint_sha256', '?'))[:16]}, the new rows come from "
                         f"{checkpoint_sha256[:16]}): one store holds the features of one checkpoint")


def append_index(path, names: Sequence[str], feats: torch.Tensor, raw: Optional[torch.Tensor] = None,
                 checkpoint_sha256: Optional[str] = None, out=None) -> int:
    """Append encoded rows to the store at `path` and write it to `out` (default: in place) -> the new number of rows.  The new
    `feats` [n,32,E] (and `raw` [n,tokens,D]) are rounded to the store's own dtypes; names already in the store, or given twice, are
    refused, and so is `checkpoint_sha256` (the fingerprint of the model that encoded the new rows) when it is not the store's.
    A store that keeps `raw` for every row needs `raw` for the new ones; one with `raw_names` takes them when given (the new names join
    `raw_names`); one without `raw` refuses them.  Runs on CPU tensors; the old rows are never re-encoded."""
    old_feats, old_raw, old_names, raw_names, meta = _read_store(path)
    _same_checkpoint(path, meta, checkpoint_sha256)
    names = list(names)
    if feats.dim() != 3 or tuple(feats.shape[1:]) != tuple(old_feats.shape[1:]) or feats.shape[0] != len(names):
        raise ValueError(f"append_index: feats {tuple(feats.shape)} for {len(names)} names, the store holds rows of {tuple(old_feats.shape[1:])}")
    dup = sorted(set(names) & set(old_names)) + sorted({n for n in names if names.count(n) > 1})
    if dup:
        raise ValueError(f"append_index: name(s) already in the store or given twice: {dup[:3]}")
    if raw is not None and (old_raw is None or raw.shape[0] != len(names) or tuple(raw.shape[1:]) != tuple(old_raw.shape[1:])):
        raise ValueError("append_index: `raw` needs a store that keeps raw embeddings, and one row of the store's shape per new name")
    if raw is None and old_raw is not None and raw_names is None and names:
        raise ValueError("append_index: the store keeps raw embeddings for every row; the new rows need `raw` too")
    new_feats = torch.cat([old_feats, feats.detach().to(old_feats.dtype).to("cpu")]) if names else old_feats
    new_raw = old_raw
    if raw is not None and names:
        new_raw = torch.cat([old_raw, raw.detach().to(old_raw.dtype).to("cpu")])
        raw_names = raw_names + names if raw_names is not None else None
    _write_store(path if out is None else out, new_feats, new_raw, old_names + names, raw_names, meta)
    return len(old_names) + len(names)


def remove_from_index(path, names: Sequence[str], checkpoint_sha256: Optional[str] = None, out=None) -> int:
    """Drop the named rows from the store at `path` and write it to `out` (default: in place) -> the number of rows left.  Unknown
    names raise KeyError; a store cannot lose its last row.  Dtypes, `raw_names` (less the dropped names) and metadata are kept."""
    feats, raw, old_names, raw_names, meta = _read_store(path)
    _same_checkpoint(path, meta, checkpoint_sha256)
    drop = set(names)
    unknown = sorted(drop - set(old_names))
    if unknown:
        raise KeyError(f"remove_from_index: not in the store: {unknown[:3]}")
    if len(drop) == len(old_names):
        raise ValueError("remove_from_index: nothing would be left")
    if drop:
        keep = torch.tensor([i for i, n in enumerate(old_names) if n not in drop], dtype=torch.long)
        feats = feats.index_select(0, keep)
        if raw is not None and raw_names is None:
            raw = raw.index_select(0, keep)
        elif raw is not None:
            rkeep = [i for i, n in enumerate(raw_names) if n not in drop]
            raw_names = [raw_names[i] for i in rkeep]
            raw = raw.index_select(0, torch.tensor(rkeep, dtype=torch.long)) if rkeep else None
            raw_names = raw_names if rkeep else None
        old_names = [n for n in old_names if n not in drop]
    _write_store(path if out is None else out, feats, raw, old_names, raw_names, meta)
    return len(old_names)
