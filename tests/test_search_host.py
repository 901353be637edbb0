"""Host side of the index search (no GPU): the 16-bit `feats` store, the segmenting rule of the two-level top-k, the directory
dataset and the command-line parser."""
import json
import struct

import numpy as np
import pytest
import torch
from PIL import Image

from sprc_amd import engine as E
from sprc_amd import index as IX


def _gallery(n=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    feats = torch.randn((n, 32, 256), generator=g)
    feats = feats / feats.norm(dim=-1, keepdim=True)
    raw = torch.randn((n, 7, 16), generator=g)
    return feats, raw, [f"img-{i}" for i in range(n)]


def _parse(path):
    """safetensors file -> (header dict, payload bytes)"""
    b = path.read_bytes()
    n = struct.unpack("<Q", b[:8])[0]
    return json.loads(b[8:8 + n]), b[8 + n:]


@pytest.mark.parametrize("dtype,name", [(torch.float16, "fp16"), (torch.bfloat16, "bf16")])
def test_feats_16bit_round_trip(tmp_path, dtype, name):
    feats, raw, names = _gallery()
    p = tmp_path / "g.safetensors"
    IX.save_index(p, feats, names, raw=raw, checkpoint_sha256="abc", feats_dtype=dtype)
    header, payload = _parse(p)
    assert header["__metadata__"]["feats_dtype"] == name
    lo, hi = header["feats"]["data_offsets"]
    want = feats.to(dtype)
    assert payload[lo:hi] == want.contiguous().view(torch.uint8).numpy().tobytes()          # the stored bytes are feats.to(dtype)
    (f, r), n, meta = IX.load_index(p)
    assert f.dtype == torch.float32 and torch.equal(f, want.float()) and n == names and meta["feats_dtype"] == name
    assert torch.equal(r, raw)
    (f16, _), _, _ = IX.load_index(p, keep_feats_dtype=True)
    assert f16.dtype == dtype and torch.equal(f16.view(torch.int16), want.view(torch.int16))
    with pytest.raises(ValueError):
        IX.save_index(p, feats, names, feats_dtype=torch.float64)


def test_default_store_is_unchanged(tmp_path):
    """The default save_index writes what the code before `feats_dtype` wrote for the same inputs: header and payload."""
    from safetensors.torch import save_file
    feats, raw, names = _gallery(seed=1)
    p, q = tmp_path / "new.safetensors", tmp_path / "old.safetensors"
    IX.save_index(p, feats, names, raw=raw, backbone="pretrain", compute_dtype="fp16", checkpoint_sha256="abc", raw_dtype=torch.float16,
                  raw_names=None)
    save_file({"feats": feats.detach().to("cpu", torch.float32).contiguous(), "raw": raw.detach().to(torch.float16).to("cpu").contiguous()}, str(q),
              metadata={"format": "sprc-index-1", "names": json.dumps(list(names)), "backbone": "pretrain", "compute_dtype": "fp16",
                        "checkpoint_sha256": "abc"})
    (header, payload), (header_q, payload_q) = _parse(p), _parse(q)
    assert header == header_q and payload == payload_q                  # (the metadata's key order inside the header is the writer's hash order)
    assert "feats_dtype" not in header["__metadata__"] and header["__metadata__"]["format"] == IX.FORMAT
    (f, _), _, meta = IX.load_index(q)                                                       # a file without the key is an fp32 store
    assert f.dtype == torch.float32 and torch.equal(f, feats) and "feats_dtype" not in meta
    (f, _), _, _ = IX.load_index(q, keep_feats_dtype=True)
    assert f.dtype == torch.float32 and torch.equal(f, feats)


def test_segmenting_rule_partitions_the_row():
    for nq in (1, 2, 3, 31, 32, 33, 70, 256, 1024, 5000):
        for N in (1, 2, 5, 63, 64, 65, 4097, 8191, 8192, 8193, 20000, 123403, 1000000, 2**31 - 1):
            for S in (None, 1, 2, 3, 7, 64, 10**7):
                seg, n_seg = E.search_segments(nq, N, S)
                assert n_seg >= 1 and seg >= 1
                assert (n_seg - 1) * seg < N <= n_seg * seg              # n_seg - 1 full segments and a last one of 1 .. seg scores cover [0, N)
                if S is not None:
                    assert n_seg <= max(1, min(S, N))
                else:
                    assert (seg, n_seg) == E.search_segments(nq, N)      # a function of (nq, N)
    assert E.search_segments(1, 5)[1] == 1 and E.search_segments(1, 123403)[1] > 1
    with pytest.raises(ValueError):
        E.search_segments(1, 0)


def test_image_dir_dataset(tmp_path):
    from sprc_amd.data_utils import ImageDirDataset
    (tmp_path / "sub").mkdir()
    for rel in ("b.png", "a.png", "sub/c.png"):
        Image.fromarray(np.zeros((5, 4, 3), dtype=np.uint8)).save(tmp_path / rel)
    (tmp_path / "notes.txt").write_text("not an image")
    ds = ImageDirDataset(tmp_path, lambda im: im.size)
    assert ds.names == ["a", "b", "c"] and len(ds) == 3
    assert ds[0] == ("a", (4, 5))
    Image.fromarray(np.zeros((5, 4, 3), dtype=np.uint8)).save(tmp_path / "sub" / "a.png")
    with pytest.raises(ValueError, match="duplicate"):
        ImageDirDataset(tmp_path, lambda im: im)
    with pytest.raises(FileNotFoundError):
        ImageDirDataset(tmp_path / "nowhere", lambda im: im)


def test_cli_parser():
    from sprc_amd.search import _parser
    p = _parser()
    a = p.parse_args(["query", "--index", "s", "--model-path", "m", "--reference", "n", "--caption", "c"])
    assert (a.command, a.reference, a.reference_image, a.k, a.json) == ("query", "n", None, 10, False)
    a = p.parse_args(["build", "--images", "d", "--model-path", "m", "--out", "o"])
    assert (a.command, a.feats_dtype, a.keep_raw, a.dtype) == ("build", "fp16", "all", "fp16")
    with pytest.raises(SystemExit):
        p.parse_args(["query", "--index", "s", "--model-path", "m", "--caption", "c"])                       # no reference form
    with pytest.raises(SystemExit):
        p.parse_args(["query", "--index", "s", "--model-path", "m", "--caption", "c", "--reference", "n", "--reference-image", "f"])
