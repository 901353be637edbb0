#!/usr/bin/env python3
"""Index search: one reference image + one caption -> the best-matching gallery names of a stored index.

    python -m sprc_amd.search build --images DIR --model-path X --out STORE [--backbone B --dtype fp16 --feats-dtype fp16
                                    --keep-raw all|none --gpu-preprocess]
    python -m sprc_amd.search query --index STORE --model-path X (--reference NAME | --reference-image FILE) --caption "..."
                                    [-k 10] [--json] [--within-file FILE | --within-glob PATTERN] [--exclude NAME...]
                                    [--exclude-reference]
    python -m sprc_amd.search batch --index STORE --model-path X --queries FILE [-k 10] [--batch 32] [--out FILE]
                                    (FILE: one JSON object per line, each with its own filters; see `parse_queries`)
    python -m sprc_amd.search add    --index STORE --images DIR --model-path X [--out STORE2]     (encodes the new stems only)
    python -m sprc_amd.search remove --index STORE --names NAME... [--out STORE2]

    s = Searcher(model, "gallery.safetensors")
    s.search(["dog-017", "/tmp/photo.jpg"], ["the same dog on a beach", "make it night"], k=10)
    shoes = s.subset(n for n in s.names if n.startswith("shoes/"))                  # uploaded once
    s.search(["dog-017"], ["in red"], k=10, within=shoes, exclude_reference=True)
    s.search(refs, caps, k=10, within_each=[dresses, None], exclude_each=[shown_a, shown_b])    # every query its own filter

No reference counterpart: the reference ranks inside its evaluation loops only (validate_blip.py:253-254).  The pieces are the
evaluation path's own -- caption processor, tokenizer, `model.fuse` -- followed by `engine.search_topk` on the store's 16-bit
`feats`: the streaming score kernel (csrc/search.hip) and the two-level top-k.  The gallery is uploaded once, when the Searcher
is made; a search does no per-gallery-item work on the host.

A filtered search (`within=`, `exclude=`, `exclude_reference=`, or after `remove`) ranks a row list instead of the whole gallery:
`engine.search_topk(rows=, exclude=)` on sprc_sim_max_stream_rows reads the listed images only.  The list is built and validated
on the host once (`resolve_rows`; `Searcher.subset` keeps it on the device for repeated searches); nothing else is per item.

Per-query filters (`within_each=`, `exclude_each=`, the `batch` command): the queries are taken in blocks of 32, each block ranks the
ascending union of its queries' sets with one admit word per listed image (`resolve_admit`), and `engine.search_topk(rows=, admit=)`
on sprc_sim_max_stream_admit reads every listed image once for the whole block.
"""
from __future__ import annotations

import fnmatch
import json
import os
import re
import time
from argparse import ArgumentParser
from pathlib import Path
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

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
    the mapping `harness._stack_refs` takes.  `extra`: the embeddings of rows added after the store was loaded, by row."""

    def __init__(self, raw, row_of: Dict[str, int]):
        self.raw, self.row_of, self.extra = raw, row_of, {}

    def get(self, name):
        i = self.row_of.get(name)
        if i is None:
            return None
        if i in self.extra:
            return self.extra[i]
        return None if self.raw is None or i >= len(self.raw) else self.raw[i]

    def __getitem__(self, name):
        r = self.get(name)
        if r is None:
            raise KeyError(name)
        return r


def _within_rows(within, n_rows: int, row_of: Dict[str, int], what: str = "within") -> List[int]:
    """`within` as `resolve_rows` takes it (not None) -> ascending, de-duplicated rows in [0, n_rows); KeyError / ValueError as there."""
    if isinstance(within, torch.Tensor):
        if within.dim() != 1 or within.is_floating_point() or within.is_complex() or within.dtype == torch.bool:
            raise ValueError(f"{what}: a tensor of rows must be one-dimensional and of an integer dtype, got {tuple(within.shape)} {within.dtype}")
        items = within.cpu().tolist()
    else:
        if isinstance(within, (str, bytes)):
            raise TypeError(f"{what}: an iterable of names or rows, not one string")
        items = list(within)
    if items and all(isinstance(i, int) and not isinstance(i, bool) for i in items):
        if items[0] < 0 or items[-1] >= n_rows or any(b <= a for a, b in zip(items, items[1:])):
            raise ValueError(f"{what}: rows must be strictly ascending values in [0, {n_rows})")
        return items
    unknown = [n for n in items if not isinstance(n, str) or n not in row_of]
    if unknown:
        raise KeyError(f"{what}: not a gallery name of this index: {unknown[:3]}")
    return sorted({row_of[n] for n in items})


def _excluded_rows(exclude, row_of: Dict[str, int], what: str = "exclude") -> set:
    exclude = [exclude] if isinstance(exclude, str) else list(exclude or ())
    unknown = [n for n in exclude if n not in row_of]
    if unknown:
        raise KeyError(f"{what}: not a gallery name of this index: {unknown[:3]}")
    return {row_of[n] for n in exclude}


def resolve_rows(within, n_rows: int, row_of: Dict[str, int], exclude: Iterable[str] = (), removed=frozenset()) -> torch.Tensor:
    """The row list of a filtered search -> int32 CPU tensor, strictly ascending, values in [0, n_rows): what `engine.search_topk(rows=)`
    trusts.  Host work only, before any device call.
    within: None (every row), an iterable of gallery names (sorted and de-duplicated here; an unknown name raises KeyError), or rows
    as an integer tensor / list of ints, which must already be strictly ascending and in range (ValueError otherwise).
    exclude: names whose rows are taken out (unknown: KeyError); removed: rows taken out.  An empty result raises ValueError."""
    rows = list(range(n_rows)) if within is None else _within_rows(within, n_rows, row_of)
    out = _excluded_rows(exclude, row_of) | set(removed)
    if out:
        rows = [i for i in rows if i not in out]
    if not rows:
        raise ValueError("the filter leaves no gallery image to rank")
    return torch.tensor(rows, dtype=torch.int32)


ADMIT_BLOCK = E.STREAM_MAX_NQ                    # queries that share one row list and one admit word per listed image


def resolve_admit(n_rows: int, row_of: Dict[str, int], within=None, exclude: Iterable[str] = (), within_each: Optional[Sequence] = None,
                  exclude_each: Optional[Sequence] = None, skip_rows: Optional[Sequence[int]] = None, removed=frozenset(),
                  first: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The row list and admit words of one block of B <= 32 queries with a filter each -> (rows int32 [M], admit int32 [M]), CPU
    tensors: what `engine.search_topk(rows=, admit=)` trusts.  Host work only, before any device call.
    Query b ranks (within & within_each[b]) - exclude - exclude_each[b] - {skip_rows[b]} - removed.  `within` and the entries of
    `within_each` are names or strictly ascending rows as `resolve_rows` takes them, None for no restriction; `exclude` and the
    entries of `exclude_each` are names, None for nothing; skip_rows[b] is a row, negative or None for none; removed: rows.
    rows is the ascending union of the B sets; bit b of admit[m] is set iff rows[m] is in query b's set (the words are uint32 bit
    patterns held as int32: query 31 is the sign bit).  B is the length of the sequences given, which must agree (ValueError).
    An unknown name raises KeyError, unsorted or out-of-range rows ValueError, and a query whose set is empty ValueError naming the
    query's position (`first` + b: the block's place in a longer call)."""
    import numpy as np
    lens = {name: len(v) for name, v in (("within_each", within_each), ("exclude_each", exclude_each), ("skip_rows", skip_rows)) if v is not None}
    if not lens:
        raise ValueError("resolve_admit: one of within_each, exclude_each and skip_rows says how many queries there are")
    B = next(iter(lens.values()))
    if any(n != B for n in lens.values()):
        raise ValueError(f"resolve_admit: one entry per query is required, got {lens}")
    if not 1 <= B <= ADMIT_BLOCK:
        raise ValueError(f"resolve_admit: a block holds 1 to {ADMIT_BLOCK} queries, got {B}")
    base = None if within is None else np.asarray(_within_rows(within, n_rows, row_of), dtype=np.int64)
    gone = _excluded_rows(exclude, row_of) | {int(i) for i in removed}
    gone = np.fromiter(sorted(gone), dtype=np.int64, count=len(gone))
    bits = np.zeros(n_rows, dtype=np.uint32)
    for b in range(B):
        wb = None if within_each is None or within_each[b] is None else within_each[b]
        if isinstance(wb, Subset):
            wb = wb.rows_cpu
        if wb is not None:
            cand = np.asarray(_within_rows(wb, n_rows, row_of, f"within_each[{first + b}]"), dtype=np.int64)
            if base is not None:
                cand = np.intersect1d(cand, base, assume_unique=True)
        else:
            cand = np.arange(n_rows, dtype=np.int64) if base is None else base
        out = gone
        eb = None if exclude_each is None else exclude_each[b]
        if eb is not None:
            each = _excluded_rows(eb, row_of, f"exclude_each[{first + b}]")
            out = np.union1d(out, np.fromiter(each, dtype=np.int64, count=len(each)))
        sb = None if skip_rows is None else skip_rows[b]
        if sb is not None and int(sb) >= 0:
            out = np.union1d(out, np.asarray([int(sb)], dtype=np.int64))
        if out.size:
            cand = cand[~np.isin(cand, out)]
        if not cand.size:
            raise ValueError(f"query {first + b}: the filter leaves no gallery image to rank")
        bits[cand] |= np.uint32(1 << b)
    rows = np.flatnonzero(bits)
    return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(bits[rows].view(np.int32).copy())


class Subset:
    """A validated row list kept on the device (`Searcher.subset`): `within=` takes it for repeated searches of one subset."""

    def __init__(self, rows_cpu: torch.Tensor, rows: torch.Tensor, edits: int):
        self.rows_cpu, self.rows, self.edits = rows_cpu, rows, edits

    def __len__(self):
        return int(self.rows_cpu.shape[0])


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
        self._removed: set = set()               # tombstoned rows: `names` keeps its numbering
        self._edits = 0                          # bumped by add / remove: device row lists made before are rebuilt
        self._live: Optional[Subset] = None      # every row that is not removed (made when the first row is removed)
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

    # ---- row lists --------------------------------------------------------------------------------------
    @property
    def row_of(self) -> Dict[str, int]:
        return self._raw.row_of

    def subset(self, within) -> Subset:
        """Resolve names (or rows) once and upload the list: the handle `within=` takes for repeated searches of the same subset."""
        rows = resolve_rows(within, len(self.names), self.row_of, removed=self._removed)
        return Subset(rows, rows.to(self.model.device), self._edits)

    def _rows(self, within, exclude) -> Optional[torch.Tensor]:
        """The device row list of one search, None for the whole gallery."""
        if isinstance(within, Subset) and not exclude:
            if within.edits != self._edits:                  # rows were added or removed since: drop the tombstones, upload again
                within.rows_cpu = resolve_rows(within.rows_cpu, len(self.names), self.row_of, removed=self._removed)
                within.rows, within.edits = within.rows_cpu.to(self.model.device), self._edits
            return within.rows
        if isinstance(within, Subset):
            within = within.rows_cpu
        if within is None and not exclude:
            if not self._removed:
                return None
            if self._live is None or self._live.edits != self._edits:
                self._live = self.subset(None)
            return self._live.rows
        return resolve_rows(within, len(self.names), self.row_of, exclude or (), self._removed).to(self.model.device)

    # ---- edits (in memory; `index.append_index` / `remove_from_index` edit the file) ------------------------
    def remove(self, names: Iterable[str]) -> None:
        """Tombstone rows: they leave every later result and can no longer be named; `names` keeps its numbering."""
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in self.row_of]
        if unknown:
            raise KeyError(f"remove: not a gallery name of this index: {unknown[:3]}")
        if len(self._removed) + len(set(names)) >= len(self.names):
            raise ValueError("remove: nothing would be left")
        for n in set(names):
            i = self.row_of.pop(n)
            self._removed.add(i)
            self._raw.extra.pop(i, None)
        self._edits += 1

    def add(self, names: Sequence[str], feats: torch.Tensor, raw: Optional[torch.Tensor] = None) -> None:
        """Append encoded rows: feats [n,32,256] (rounded to the rank dtype), raw [n,tokens,D] (optional: the embeddings that let the
        new images be references).  Names of the gallery, or given twice, are refused.  The device tensor grows by doubling."""
        names = list(names)
        if feats.dim() != 3 or feats.shape[0] != len(names) or tuple(feats.shape[1:]) != tuple(self.feats.shape[1:]):
            raise ValueError(f"add: feats {tuple(feats.shape)} for {len(names)} names, the gallery holds rows of {tuple(self.feats.shape[1:])}")
        if raw is not None and raw.shape[0] != len(names):
            raise ValueError("add: one row of `raw` per name")
        dup = [n for n in names if n in self.row_of] + sorted({n for n in names if names.count(n) > 1})
        if dup:
            raise ValueError(f"add: name(s) already in the gallery or given twice: {dup[:3]}")
        if not names:
            return
        n0, n1 = self.feats.shape[0], self.feats.shape[0] + len(names)
        buf = getattr(self, "_buf", None)
        if buf is None or buf.data_ptr() != self.feats.data_ptr() or buf.shape[0] < n1:
            buf = torch.empty((max(2 * n0, n1),) + tuple(self.feats.shape[1:]), dtype=self.feats.dtype, device=self.feats.device)
            buf[:n0] = self.feats
            self._buf = buf
        buf[n0:n1] = feats.to(device=buf.device, dtype=buf.dtype)
        self.feats = buf[:n1]
        for j, n in enumerate(names):
            self.row_of[n] = n0 + j
            if raw is not None:
                self._raw.extra[n0 + j] = raw[j].to(self.model.device).float()
        self.names.extend(names)
        self._edits += 1

    @torch.no_grad()
    def add_images(self, files: Sequence) -> List[str]:
        """Encode image files (the gallery's transform, `model.extract_target_features`) and `add` them under their stems."""
        from PIL import Image
        files = [Path(f) for f in files]
        names = [f.stem for f in files]
        if not files:
            return names
        images = torch.stack([self.preprocess(Image.open(f)) for f in files])
        with torch.cuda.device(self.model.device):
            feats, raw = self.model.extract_target_features(images.to(self.model.device, torch.float32))
            self.add(names, feats, raw)
        return names

    # ---- search -------------------------------------------------------------------------------------
    @torch.no_grad()
    def search_ids(self, reference, input_ids: torch.Tensor, attention_mask: torch.Tensor, k: int,
                   timings: Optional[dict] = None, within=None, exclude: Optional[Iterable[str]] = None,
                   exclude_reference: bool = False, within_each: Optional[Sequence] = None,
                   exclude_each: Optional[Sequence] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (scores [B,k] fp32, gallery rows [B,k] int32; -inf / -1 beyond the gallery's size).  timings: a dict that receives
        the milliseconds of the three phases (reference embeddings, fuse, rank), each ended by a device synchronisation.
        within: names, rows (int tensor / list, strictly ascending) or a `subset` handle -- only these are ranked; exclude: names
        left out for every query; exclude_reference: a query's reference is left out when it is a gallery name.  A filtered search
        (any of the three, or rows removed earlier) runs `engine.search_topk(rows=, exclude=)` for any number of queries.
        within_each / exclude_each: one entry per query (None: no restriction / nothing excluded), combined with the shared filters;
        with either, the queries are ranked in blocks of 32 by `engine.search_topk(rows=, admit=)` (`_search_each`)."""
        if within_each is not None or exclude_each is not None:
            return self._search_each(reference, input_ids, attention_mask, k, timings, within, exclude, exclude_reference, within_each,
                                     exclude_each)
        dev = self.model.device

        def lap(key, t0):
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings[key] = (time.perf_counter() - t0) * 1e3
            return time.perf_counter()

        if isinstance(reference, (str, Path, torch.Tensor)):
            reference = [reference]
        reference = list(reference)
        rows = self._rows(within, exclude)                                   # host: raises before any device work
        skip = None
        if exclude_reference:
            skip = [self.row_of.get(r, -1) if isinstance(r, str) else -1 for r in reference]
            skip = torch.tensor(skip, dtype=torch.int32) if any(i >= 0 for i in skip) else None
        t = time.perf_counter()
        with torch.cuda.device(dev):
            ref = self.reference_embeds(reference)
            if ref.shape[0] != input_ids.shape[0]:
                raise ValueError("one caption per reference image is required")
            t = lap("reference_ms", t)
            fusion = self.model.fuse(ref, input_ids.to(dev), attention_mask.to(dev))
            fusion = fusion.to(self.rank_dtype).contiguous()
            t = lap("fuse_ms", t)
            if rows is not None or skip is not None:
                if skip is not None and skip.shape[0] != fusion.shape[0]:
                    raise ValueError("exclude_reference: one reference per query is required")
                vals, idx = E.search_topk(fusion, self.feats, k, rows=rows, exclude=skip)
            elif fusion.shape[0] <= STREAM_MAX_QUERIES:
                vals, idx = E.search_topk(fusion, self.feats, k)
            else:
                sim = E.sim_max(fusion, self.feats, out=E.segmented_sim_buffer(fusion.shape[0], self.feats.shape[0], dev))
                vals, idx = E.topk_segmented(sim, k)
            lap("rank_ms", t)
        return vals, idx

    def _search_each(self, reference, input_ids, attention_mask, k, timings, within, exclude, exclude_reference, within_each, exclude_each):
        """`search_ids` with a filter per query.  Block by block of 32 queries: the ascending union of the block's sets and one admit
        word per listed image (`resolve_admit`, every block before any device call), then one `engine.search_topk(rows=, admit=)`
        per block.  The unions are per block on purpose: with disjoint per-query lists, a union over hundreds of queries would make
        every block walk every list.  The reference to leave out and the removed rows are bits of the admit words here."""
        dev = self.model.device
        if isinstance(reference, (str, Path, torch.Tensor)):
            reference = [reference]
        reference = list(reference)
        B = len(reference)
        for name, each in (("within_each", within_each), ("exclude_each", exclude_each)):
            if each is not None and (isinstance(each, (str, bytes)) or len(each) != B):
                raise ValueError(f"{name}: one entry per query is required ({B} queries)")
        if input_ids.shape[0] != B:
            raise ValueError("one caption per reference image is required")
        if isinstance(within, Subset):
            within = within.rows_cpu
        skip = [self.row_of.get(r, -1) if exclude_reference and isinstance(r, str) else -1 for r in reference]
        blocks = []
        for b0 in range(0, B, ADMIT_BLOCK):
            cut = slice(b0, min(b0 + ADMIT_BLOCK, B))
            blocks.append(resolve_admit(len(self.names), self.row_of, within, exclude or (), None if within_each is None else list(within_each[cut]),
                                        None if exclude_each is None else list(exclude_each[cut]), skip[cut], self._removed, first=b0))
        t = time.perf_counter()
        with torch.cuda.device(dev):
            ref = self.reference_embeds(reference)
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings["reference_ms"], t = (time.perf_counter() - t) * 1e3, time.perf_counter()
            fusion = self.model.fuse(ref, input_ids.to(dev), attention_mask.to(dev)).to(self.rank_dtype).contiguous()
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings["fuse_ms"], t = (time.perf_counter() - t) * 1e3, time.perf_counter()
            out = []
            for i, (rows, admit) in enumerate(blocks):
                b0 = i * ADMIT_BLOCK
                out.append(E.search_topk(fusion[b0:b0 + ADMIT_BLOCK], self.feats, k, rows=rows.to(dev), admit=admit.to(dev).view(1, -1)))
            vals, idx = (out[0] if len(out) == 1 else (torch.cat([v for v, _ in out]), torch.cat([i for _, i in out])))
            if timings is not None:
                torch.cuda.synchronize(dev)
                timings["rank_ms"] = (time.perf_counter() - t) * 1e3
        return vals, idx

    def search(self, reference, captions: Union[str, Sequence[str]], k: int = 10, timings: Optional[dict] = None, within=None,
               exclude: Optional[Iterable[str]] = None, exclude_reference: bool = False, within_each: Optional[Sequence] = None,
               exclude_each: Optional[Sequence] = None) -> List[List[Tuple[str, float]]]:
        if isinstance(captions, str):
            captions = [captions]
        text = [self.txt_processors["eval"](c) for c in captions]
        tok = self.model.tokenizer(text, padding="max_length", truncation=True, max_length=self.model.max_txt_len, return_tensors="pt")
        vals, idx = self.search_ids(reference, tok.input_ids, tok.attention_mask, k, timings=timings, within=within, exclude=exclude,
                                    exclude_reference=exclude_reference, within_each=within_each, exclude_each=exclude_each)
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
    within = q.add_mutually_exclusive_group()
    within.add_argument("--within-file", type=str, help="rank only the gallery names listed in this file, one per line")
    within.add_argument("--within-glob", type=str, help="rank only the gallery names that match this pattern (fnmatch)")
    q.add_argument("--exclude", type=str, nargs="+", default=None, help="gallery names left out of the ranking")
    q.add_argument("--exclude-reference", action="store_true", help="leave the reference out when it is a gallery name")
    common(q)
    bt = sub.add_parser("batch", help="answer a file of queries, each with its own filters, with the model and the store loaded once")
    bt.add_argument("--index", type=str, required=True)
    bt.add_argument("--queries", type=str, required=True, help="one JSON object per line: reference | reference_image, caption, "
                    "within, within_glob, exclude, exclude_reference")
    bt.add_argument("-k", type=int, default=10)
    bt.add_argument("--batch", type=int, default=ADMIT_BLOCK, help=f"queries answered per call, 1 to {ADMIT_BLOCK}")
    bt.add_argument("--out", type=str, default=None, help="write the JSON lines here instead of to stdout")
    common(bt)
    ad = sub.add_parser("add", help="encode the image files whose stem is not yet a name of the store and append them")
    ad.add_argument("--index", type=str, required=True)
    ad.add_argument("--images", type=str, required=True, help="directory of image files; a file's stem is its gallery name")
    ad.add_argument("--out", type=str, default=None, help="write here instead of rewriting --index")
    common(ad)
    rm = sub.add_parser("remove", help="drop named rows from a store")
    rm.add_argument("--index", type=str, required=True)
    rm.add_argument("--names", type=str, nargs="+", required=True)
    rm.add_argument("--out", type=str, default=None, help="write here instead of rewriting --index")
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
    within = None
    if a.within_file is not None:
        within = [l.strip() for l in Path(a.within_file).read_text().splitlines() if l.strip()]
    elif a.within_glob is not None:
        within = [n for n in s.names if fnmatch.fnmatchcase(n, a.within_glob)]
        if not within:
            raise ValueError(f"--within-glob {a.within_glob!r} matches no gallery name")
    hits = s.search([a.reference if a.reference is not None else Path(a.reference_image)], [a.caption], k=a.k, timings=timings,
                    within=within, exclude=a.exclude, exclude_reference=a.exclude_reference)[0]
    if a.json:
        print(json.dumps({"caption": a.caption, "reference": a.reference or a.reference_image, "timings": timings,
                          "results": [{"rank": r + 1, "name": n, "score": v} for r, (n, v) in enumerate(hits)]}))
    else:
        for r, (n, v) in enumerate(hits):
            print(f"{r + 1:4d}  {n}  {v:.6f}")
    return hits


_QUERY_KEYS = {"reference", "reference_image", "caption", "within", "within_glob", "exclude", "exclude_reference"}


def parse_queries(text: str) -> List[dict]:
    """The lines of a `batch` file -> one dict per query: line (1-based), reference (a gallery name) or reference_image (a path),
    caption, within (names or None), within_glob (pattern or None), exclude (names or None), exclude_reference (bool).  Blank lines
    are skipped.  Host work only; a ValueError names the line."""
    out = []
    for no, raw in enumerate(text.splitlines(), 1):
        if not raw.strip():
            continue
        try:
            o = json.loads(raw)
        except json.JSONDecodeError as e:
            raise ValueError(f"line {no}: not JSON ({e.msg} at column {e.colno})") from None
        if not isinstance(o, dict):
            raise ValueError(f"line {no}: a JSON object is required")
        if set(o) - _QUERY_KEYS:
            raise ValueError(f"line {no}: unknown key(s) {sorted(set(o) - _QUERY_KEYS)}")
        if not isinstance(o.get("caption"), str):
            raise ValueError(f"line {no}: \"caption\" (a string) is required")
        if ("reference" in o) == ("reference_image" in o):
            raise ValueError(f"line {no}: exactly one of \"reference\" and \"reference_image\" is required")
        key = "reference" if "reference" in o else "reference_image"
        if not isinstance(o[key], str):
            raise ValueError(f"line {no}: \"{key}\" must be a string")
        for key in ("within", "exclude"):
            if o.get(key) is not None and not (isinstance(o[key], list) and all(isinstance(n, str) for n in o[key])):
                raise ValueError(f"line {no}: \"{key}\" must be a list of gallery names")
        if o.get("within_glob") is not None and not isinstance(o["within_glob"], str):
            raise ValueError(f"line {no}: \"within_glob\" must be a string")
        if not isinstance(o.get("exclude_reference", False), bool):
            raise ValueError(f"line {no}: \"exclude_reference\" must be true or false")
        out.append(dict(line=no, reference=o.get("reference"), reference_image=o.get("reference_image"), caption=o["caption"],
                        within=o.get("within"), within_glob=o.get("within_glob"), exclude=o.get("exclude"),
                        exclude_reference=o.get("exclude_reference", False)))
    return out


def query_filters(entry: dict, names: Sequence[str], row_of: Dict[str, int]) -> Tuple[Optional[List[str]], Optional[List[str]]]:
    """One parsed `batch` line against a store's names -> (within, exclude) as `Searcher.search(within_each=, exclude_each=)` takes
    them, None for "no restriction" / "nothing excluded".  within and within_glob together mean the listed names that match;
    exclude_reference adds a stored reference to exclude.  Host work only; a KeyError / ValueError names the line."""
    no = entry["line"]
    if entry["reference"] is not None and entry["reference"] not in row_of:
        raise KeyError(f"line {no}: reference {entry['reference']!r} is not a gallery name of this index")
    for key in ("within", "exclude"):
        unknown = [n for n in entry[key] or () if n not in row_of]
        if unknown:
            raise KeyError(f"line {no}: {key}: not a gallery name of this index: {unknown[:3]}")
    within = entry["within"]
    if entry["within_glob"] is not None:
        within = [n for n in (names if within is None else within) if n in row_of and fnmatch.fnmatchcase(n, entry["within_glob"])]
        if not within:
            raise ValueError(f"line {no}: within_glob {entry['within_glob']!r} matches no gallery name")
    exclude = list(entry["exclude"] or ())
    if entry["exclude_reference"] and entry["reference"] is not None:
        exclude.append(entry["reference"])
    return within, exclude or None


def batch_index(a) -> List[List[Tuple[str, float]]]:
    """`batch`: the whole file is parsed before anything is loaded; every line's filter is resolved against the store's names before
    the first search; then the lines are answered `--batch` at a time.  A batch without any filter takes the unfiltered path."""
    if not 1 <= a.batch <= ADMIT_BLOCK:
        raise ValueError(f"--batch {a.batch}: 1 to {ADMIT_BLOCK} queries per call")
    entries = parse_queries(Path(a.queries).read_text())
    from .blip_validate import _load, _preprocess
    model, _ = _load(MODEL_NAME, a.backbone, a.model_path, a.dtype, a.vit_depth)
    s = Searcher(model, a.index, preprocess=_preprocess(a.gpu_preprocess, model.device)[0])
    filters = [query_filters(e, s.names, s.row_of) for e in entries]
    hits: List[List[Tuple[str, float]]] = []
    for b0 in range(0, len(entries), a.batch):
        part, flt = entries[b0:b0 + a.batch], filters[b0:b0 + a.batch]
        refs = [e["reference"] if e["reference"] is not None else Path(e["reference_image"]) for e in part]
        caps = [e["caption"] for e in part]
        try:
            if all(w is None and x is None for w, x in flt):
                hits += s.search(refs, caps, k=a.k)
            else:
                hits += s.search(refs, caps, k=a.k, within_each=[w for w, _ in flt], exclude_each=[x for _, x in flt])
        except ValueError as e:                                  # "query b: the filter leaves ...": say which line that is
            m = re.match(r"query (\d+): (.*)", str(e))
            if m is None:
                raise
            raise ValueError(f"line {part[int(m.group(1))]['line']}: {m.group(2)}") from None
    lines = [json.dumps({"line": e["line"], "caption": e["caption"], "reference": e["reference"] or e["reference_image"],
                         "results": [{"rank": r + 1, "name": n, "score": v} for r, (n, v) in enumerate(h)]}) for e, h in zip(entries, hits)]
    if a.out is not None:
        Path(a.out).write_text("".join(l + "\n" for l in lines))
    else:
        for l in lines:
            print(l)
    return hits


def add_to_index(a) -> dict:
    """Encode the files under --images whose stem the store does not hold yet and append them (`index.append_index`)."""
    from .blip_validate import _load, _preprocess, model_fingerprint
    from .data_utils import ImageDirDataset
    from .harness import extract_index_blip_features
    from .index import _read_store, append_index
    _, old_raw, old_names, _, meta = _read_store(a.index)
    model, _ = _load(MODEL_NAME, a.backbone, a.model_path, a.dtype, a.vit_depth)
    fp = model_fingerprint(model)
    if meta.get("checkpoint_sha256") != fp:
        raise ValueError(f"{a.index}: written by another checkpoint ({str(meta.get('checkpoint_sha256', '?'))[:16]}, this model is {fp[:16]})")
    preprocess, workers = _preprocess(a.gpu_preprocess, model.device)
    dataset = ImageDirDataset(a.images, preprocess)
    have = set(old_names)
    new = [i for i, n in enumerate(dataset.names) if n not in have]
    dataset.paths, dataset.names = [dataset.paths[i] for i in new], [dataset.names[i] for i in new]
    total = len(old_names)
    if new:
        keep = old_raw is not None
        (feats, raw), names = extract_index_blip_features(dataset, model, num_workers=workers if len(dataset) >= 256 else 0, keep_raw=keep)
        if len(names) != len(dataset):
            raise SystemExit(f"search add: {len(dataset) - len(names)} of {len(dataset)} files could not be read")
        total = append_index(a.index, names, feats, raw=raw if keep else None, checkpoint_sha256=fp, out=a.out)
    elif a.out is not None:
        total = append_index(a.index, [], torch.empty((0, 32, 256)), checkpoint_sha256=fp, out=a.out)
    out = {"index": str(a.out or a.index), "added": len(new), "images": total}
    print(json.dumps(out))
    return out


def remove_from_store(a) -> dict:
    from .index import remove_from_index
    total = remove_from_index(a.index, a.names, out=a.out)
    out = {"index": str(a.out or a.index), "removed": len(set(a.names)), "images": total}
    print(json.dumps(out))
    return out


def main(argv=None):
    a = _parser().parse_args(argv)
    return {"build": build_index, "query": query_index, "batch": batch_index, "add": add_to_index, "remove": remove_from_store}[a.command](a)


if __name__ == "__main__":
    main()
