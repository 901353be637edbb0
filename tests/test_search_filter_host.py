"""Host side of the filtered index search (no GPU): the row list a filtered search ranks (`search.resolve_rows`), the two file edits
(`index.append_index`, `index.remove_from_index`) on CPU tensors, and the command-line parser's new flags and sub-commands."""
import json
import struct

import pytest
import torch

from sprc_amd import index as IX
from sprc_amd import search as SR

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


def _gallery(n=6, seed=0, first=0):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn((n, 32, 256), generator=g)
    feats = feats / feats.norm(dim=-1, keepdim=True)
    raw = torch.randn((n, 7, 16), generator=g)
    return feats, raw, [f"img-{first + i}" for i in range(n)]


def _parse(path):
    """safetensors file -> (header dict, payload bytes); the metadata's key order inside the header is the writer's hash order"""
    b = path.read_bytes()
    n = struct.unpack("<Q", b[:8])[0]
    return json.loads(b[8:8 + n]), b[8 + n:]


# ---- the row list -------------------------------------------------------------------------------------------------------------------
def test_resolve_rows_sorts_and_deduplicates_names():
    names = [f"n{i}" for i in range(10)]
    row_of = {n: i for i, n in enumerate(names)}
    r = SR.resolve_rows(["n7", "n2", "n7", "n0", "n2"], 10, row_of)
    assert r.dtype == torch.int32 and r.device.type == "cpu" and r.tolist() == [0, 2, 7]
    assert SR.resolve_rows(None, 10, row_of).tolist() == list(range(10))
    assert SR.resolve_rows((n for n in names if n > "n5"), 10, row_of).tolist() == [6, 7, 8, 9]               # any iterable
    assert SR.resolve_rows(None, 10, row_of, exclude=["n3"], removed={0, 9}).tolist() == [1, 2, 4, 5, 6, 7, 8]
    assert SR.resolve_rows(["n3", "n4"], 10, row_of, exclude=["n3", "n8"]).tolist() == [4]
    assert SR.resolve_rows(torch.tensor([1, 4, 9]), 10, row_of).tolist() == [1, 4, 9]
    assert SR.resolve_rows(torch.tensor([1, 4, 9], dtype=torch.int32), 10, row_of, removed={4}).tolist() == [1, 9]
    assert SR.resolve_rows([0, 5], 10, row_of).tolist() == [0, 5]


def test_resolve_rows_refusals():
    names = [f"n{i}" for i in range(10)]
    row_of = {n: i for i, n in enumerate(names)}
    with pytest.raises(KeyError):
        SR.resolve_rows(["n1", "nope"], 10, row_of)
    with pytest.raises(KeyError):
        SR.resolve_rows(None, 10, row_of, exclude=["nope"])
    with pytest.raises(KeyError):
        SR.resolve_rows(["n1", 3], 10, row_of)                                    # names and rows are not mixed
    for empty in ([], torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError):
            SR.resolve_rows(empty, 10, row_of)
    with pytest.raises(ValueError):
        SR.resolve_rows(["n1"], 10, row_of, exclude=["n1"])                        # everything filtered away
    with pytest.raises(ValueError):
        SR.resolve_rows(["n1"], 10, row_of, removed={1})
    for bad in ([3, 2], [2, 2], [-1, 2], [0, 10], [10]):                           # unsorted, repeated, out of range
        with pytest.raises(ValueError):
            SR.resolve_rows(torch.tensor(bad), 10, row_of)
        with pytest.raises(ValueError):
            SR.resolve_rows(bad, 10, row_of)
    with pytest.raises(ValueError):
        SR.resolve_rows(torch.tensor([0.0, 1.0]), 10, row_of)
    with pytest.raises(ValueError):
        SR.resolve_rows(torch.tensor([[0, 1]]), 10, row_of)
    with pytest.raises(TypeError):
        SR.resolve_rows("n1", 10, row_of)


# ---- the file edits -----------------------------------------------------------------------------------------------------------------
def _store(tmp_path, feats_dtype, raw_mode, n=6):
    feats, raw, names = _gallery(n)
    kw = dict(backbone="pretrain", compute_dtype="fp16", checkpoint_sha256="abc", feats_dtype=DTYPES[feats_dtype])
    p = tmp_path / f"s-{feats_dtype}-{raw_mode}.safetensors"
    if raw_mode == "none":
        IX.save_index(p, feats, names, **kw)
    elif raw_mode == "all":
        IX.save_index(p, feats, names, raw=raw, raw_dtype=torch.float16, **kw)
    else:                                                                         # embeddings of rows 4 and 1 only, in that order
        IX.save_index(p, feats, names, raw=raw[[4, 1]], raw_dtype=torch.bfloat16, raw_names=[names[4], names[1]], **kw)
    return p, feats, raw, names


@pytest.mark.parametrize("raw_mode", ["none", "all", "subset"])
@pytest.mark.parametrize("feats_dtype", ["fp16", "bf16", "fp32"])
def test_append_and_remove_keep_the_store(tmp_path, feats_dtype, raw_mode):
    p, feats, raw, names = _store(tmp_path, feats_dtype, raw_mode)
    f2, r2, n2 = _gallery(3, seed=9, first=100)
    before = _parse(p)
    meta0 = before[0]["__metadata__"]
    out = tmp_path / "out.safetensors"
    total = IX.append_index(p, n2, f2, raw=None if raw_mode == "none" else r2, checkpoint_sha256="abc", out=out)
    assert total == 9 and _parse(p) == before                                     # --out: the source is not touched
    header, _ = _parse(out)
    meta = header["__metadata__"]
    assert set(meta) == set(meta0) and all(meta[k] == meta0[k] for k in meta0 if k not in ("names", "raw_names"))
    assert header["feats"]["dtype"] == before[0]["feats"]["dtype"] and header["feats"]["shape"] == [9, 32, 256]
    assert ("raw" in header) == (raw_mode != "none")
    if raw_mode != "none":
        assert header["raw"]["dtype"] == before[0]["raw"]["dtype"]
    dt = DTYPES[feats_dtype]
    (f, r), n, m = IX.load_index(out, keep_feats_dtype=True)
    assert n == names + n2 and f.dtype == dt and m.get("feats_dtype") == (None if feats_dtype == "fp32" else feats_dtype)
    assert torch.equal(f[:6], feats.to(dt)) and torch.equal(f[6:], f2.to(dt))     # old rows bit for bit, new rows rounded to the store's dtype
    if raw_mode == "all":
        assert torch.equal(r, torch.cat([raw, r2]).to(torch.float16).float())
    elif raw_mode == "subset":
        assert json.loads(meta["raw_names"]) == [names[4], names[1]] + n2
        assert r.kept == 5 and torch.equal(r[4], raw[4].to(torch.bfloat16).float()) and torch.equal(r[7], r2[1].to(torch.bfloat16).float())
        assert r[0] is None
    # remove, in place: two old rows (one of them kept in a raw subset) and one new row
    left = IX.remove_from_index(out, [names[4], names[0], n2[1]], checkpoint_sha256="abc")
    keep = [1, 2, 3, 5, 6, 8]
    (f, r), n, m = IX.load_index(out, keep_feats_dtype=True)
    assert left == 6 and n == [(names + n2)[i] for i in keep] and f.dtype == dt
    assert torch.equal(f, torch.cat([feats, f2]).to(dt)[keep])
    header2, _ = _parse(out)
    assert set(header2["__metadata__"]) == set(meta0) and header2["feats"]["dtype"] == before[0]["feats"]["dtype"]
    if raw_mode == "all":
        assert torch.equal(r, torch.cat([raw, r2]).to(torch.float16).float()[keep])
    elif raw_mode == "subset":
        assert json.loads(header2["__metadata__"]["raw_names"]) == [names[1], n2[0], n2[2]]
        assert r.kept == 3 and torch.equal(r[0], raw[1].to(torch.bfloat16).float()) and torch.equal(r[5], r2[2].to(torch.bfloat16).float())


@pytest.mark.parametrize("raw_mode", ["none", "all", "subset"])
@pytest.mark.parametrize("feats_dtype", ["fp16", "bf16", "fp32"])
def test_edits_of_nothing_rewrite_the_same_file(tmp_path, feats_dtype, raw_mode):
    """No row gained or lost: header (as a dict: the metadata's key order is the writer's hash order) and payload are what the file
    held, through either function, as they are through a load and save of the file's own contents."""
    p, _, _, _ = _store(tmp_path, feats_dtype, raw_mode)
    want = _parse(p)
    a, b = tmp_path / "a.safetensors", tmp_path / "b.safetensors"
    assert IX.append_index(p, [], torch.empty((0, 32, 256)), out=a) == 6
    assert IX.remove_from_index(p, [], out=b) == 6
    assert _parse(a) == want and _parse(b) == want and _parse(p) == want
    IX.remove_from_index(p, [])                                                   # in place
    assert _parse(p) == want


def test_edit_refusals(tmp_path):
    p, feats, raw, names = _store(tmp_path, "fp16", "all")
    f2, r2, n2 = _gallery(2, seed=3, first=50)
    want = _parse(p)
    with pytest.raises(ValueError, match="another checkpoint"):
        IX.append_index(p, n2, f2, raw=r2, checkpoint_sha256="other")
    with pytest.raises(ValueError, match="another checkpoint"):
        IX.remove_from_index(p, [names[0]], checkpoint_sha256="other")
    with pytest.raises(ValueError, match="already in the store"):
        IX.append_index(p, [names[2], "new"], f2, raw=r2)
    with pytest.raises(ValueError, match="given twice"):
        IX.append_index(p, ["new", "new"], f2, raw=r2)
    with pytest.raises(ValueError):
        IX.append_index(p, n2, f2)                                                # the store keeps raw for every row
    with pytest.raises(ValueError):
        IX.append_index(p, n2, f2[:1], raw=r2)                                    # one row per name
    with pytest.raises(ValueError):
        IX.append_index(p, n2, f2[:, :16], raw=r2)
    with pytest.raises(KeyError):
        IX.remove_from_index(p, ["nope"])
    with pytest.raises(ValueError):
        IX.remove_from_index(p, names)                                            # nothing left
    q, _, _, _ = _store(tmp_path, "fp16", "none")
    with pytest.raises(ValueError):
        IX.append_index(q, n2, f2, raw=r2)                                        # a store without raw takes none
    assert _parse(p) == want                                                      # a refused edit writes nothing
    other = tmp_path / "not-an-index.safetensors"
    from safetensors.torch import save_file
    save_file({"feats": feats}, str(other), metadata={"format": "something-else"})
    with pytest.raises(ValueError):
        IX.remove_from_index(other, [])


# ---- the parser ---------------------------------------------------------------------------------------------------------------------
def test_parser_filter_flags_and_edit_commands(capsys):
    P = SR._parser()
    base = ["query", "--index", "s", "--model-path", "m", "--reference", "r", "--caption", "c"]
    a = P.parse_args(base)
    assert a.within_file is None and a.within_glob is None and a.exclude is None and a.exclude_reference is False
    a = P.parse_args(base + ["--within-glob", "item-00*", "--exclude", "x", "y", "--exclude-reference"])
    assert a.within_glob == "item-00*" and a.exclude == ["x", "y"] and a.exclude_reference is True
    assert P.parse_args(base + ["--within-file", "list.txt"]).within_file == "list.txt"
    with pytest.raises(SystemExit):
        P.parse_args(base + ["--within-file", "f", "--within-glob", "g"])         # one subset per query
    a = P.parse_args(["add", "--index", "s", "--images", "d", "--model-path", "m", "--vit-depth", "1", "--out", "t"])
    assert (a.command, a.index, a.images, a.out, a.model_path, a.vit_depth, a.dtype) == ("add", "s", "d", "t", "m", 1, "fp16")
    assert P.parse_args(["add", "--index", "s", "--images", "d", "--model-path", "m"]).out is None
    a = P.parse_args(["remove", "--index", "s", "--names", "x", "y"])
    assert (a.command, a.index, a.names, a.out) == ("remove", "s", ["x", "y"], None)
    for bad in (["add", "--index", "s", "--model-path", "m"], ["remove", "--index", "s"], ["remove", "--names", "x"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    capsys.readouterr()


def test_remove_command_runs_without_a_model(tmp_path, capsys):
    p, feats, _, names = _store(tmp_path, "fp16", "all")
    out = tmp_path / "smaller.safetensors"
    res = SR.main(["remove", "--index", str(p), "--names", names[2], names[5], "--out", str(out)])
    assert res == {"index": str(out), "removed": 2, "images": 4} and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    (f, _), n, _ = IX.load_index(out, keep_feats_dtype=True)
    assert n == [names[i] for i in (0, 1, 3, 4)] and torch.equal(f, feats.to(torch.float16)[[0, 1, 3, 4]])
