"""Index search on the GPU: the streaming score kernel (sprc_sim_max_stream), the two-level top-k (E.search_topk) and the
`sprc_amd.search` interface end to end.

Every raw call of the kernel writes into a score buffer with ld_sim > N inside a sentinel-filled allocation (tests/_train_ref.py:
Guard) whose bits outside sim[q < nq, 0..N) are compared afterwards.  Bars:
  * exact data (integers in [-8, 8] x 2^-6: every product a multiple of 2^-12, every 256-term sum below 4, so fp32 accumulation is
    exact in any order): bit-equal to a float64 numpy evaluation and to E.sim_max;
  * random unit-norm rows: every feature row's score is a sum of 256 fp32 terms, |s~_j - s_j| <= b_j = 2 256 2^-24 sum_k|q_k f_jk| +
    1 ulp, so the kernel's max lies in [max_j (s_j - b_j), max_j (s_j + b_j)], and within b of s at the arg-max row
    wherever no other row comes within its own bound of it;
  * search_topk: bit-identical to the single-level E.topk / E.topk_wide on the stream kernel's own scores, for every segmenting.
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from _train_ref import strided  # noqa: E402
from sprc_amd import _lib as L  # noqa: E402
from sprc_amd import engine as E  # noqa: E402

DEV = "cuda:0"
DTYPES = {"fp16": (torch.float16, L.SPRC_F16), "bf16": (torch.bfloat16, L.SPRC_BF16)}
P = E.STREAM_P


def _stream_raw(fusion, feats, nq, N, dt, ld_extra=5, E_=256, ld=None, ptr_shift=(0, 0)):
    """One raw sprc_sim_max_stream call into a guarded buffer -> (rc, guard, logical sim view)."""
    lib = L.load()
    ld = N + ld_extra if ld is None else ld
    g, sim = strided(max(nq, 1), max(N, 1), max(ld, max(N, 1)), device=DEV)
    g.seal()
    rc = lib.sprc_sim_max_stream(None if fusion is None else fusion.data_ptr() + ptr_shift[0], None if feats is None else feats.data_ptr() + ptr_shift[1],
                                 sim.data_ptr(), ld, nq, N, E_, dt, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, g, sim


def _grid():
    return E.STREAM_WG_PER_CU * L.load().sprc_stream_cus(None)


_EXACT = {}


def _exact_case(N):
    """(queries [32,256], gallery [N,32,256]) as float32 holding integers in [-8, 8] x 2^-6, and the float64 scores [32, N]."""
    if N not in _EXACT:
        rng = np.random.default_rng(1000 + N)
        q = rng.integers(-8, 9, size=(32, 256)).astype(np.float64) / 64.0
        f = rng.integers(-8, 9, size=(N, 32, 256)).astype(np.float64) / 64.0
        ref = (f.reshape(N * 32, 256) @ q.T).reshape(N, 32, 32).max(axis=1).T.copy()        # [q, n], float64
        _EXACT[N] = (torch.from_numpy(q.astype(np.float32)), torch.from_numpy(f.astype(np.float32)), ref)
    return _EXACT[N]


def _exact_sizes():
    return [1, 2, 63, 64, 65, P - 1, P, P + 1, 3 * P + 5, "ragged"]


@pytest.mark.parametrize("N", _exact_sizes())
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_stream_exact(dtype, N):
    """Exact operands: bit-equal to float64 and to the GEMM path, nothing written outside sim[q < nq, 0..N)."""
    if N == "ragged":                     # more trips than workgroups and not a multiple: every workgroup takes 2 or 3 trips, the last one is short
        N = P * (2 * _grid() + 3) + 5
    tdt, sdt = DTYPES[dtype]
    q32, f32, ref = _exact_case(N)
    feats = f32.to(DEV).to(tdt).contiguous()
    assert torch.equal(feats.float().cpu(), f32)                     # the operands are exact in both 16-bit formats
    for nq in (1, 2, 31, 32):
        fusion = q32[:nq].to(DEV).to(tdt).contiguous()
        rc, g, sim = _stream_raw(fusion, feats, nq, N, sdt)
        assert rc == 0, L.load().sprc_last_error()
        assert g.outside_intact(), (dtype, nq, N)
        got = sim.cpu().numpy()
        want = ref[:nq].astype(np.float32)
        assert np.array_equal(want.astype(np.float64), ref[:nq])     # the float64 scores are fp32 numbers
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dtype, nq, N, np.abs(got - want).max())
        gemm = E.sim_max(fusion, feats)
        assert torch.equal(sim.contiguous().view(torch.int32), gemm.view(torch.int32)), (dtype, nq, N)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_stream_layout_probes(dtype):
    """One 1 per image at feats[n = (j, c), j, 8 c + e], query slot (5 c + 3) % 32 = e_{8 c + e}: sim is exactly 1.0 where the image's
    chunk c is the slot's and 0.0 elsewhere, for every feature row j, every 8-element chunk c and every element e of a chunk."""
    tdt, sdt = DTYPES[dtype]
    N = 32 * 32
    j, c = torch.arange(32).repeat_interleave(32), torch.arange(32).repeat(32)
    slot = (5 * torch.arange(32) + 3) % 32
    want = torch.zeros((32, N))
    want[slot[c], torch.arange(N)] = 1.0
    for e in range(8):
        feats = torch.zeros((N, 32, 256))
        feats[torch.arange(N), j, 8 * c + e] = 1.0
        fusion = torch.zeros((32, 256))
        fusion[slot, 8 * torch.arange(32) + e] = 1.0
        rc, g, sim = _stream_raw(fusion.to(DEV).to(tdt), feats.to(DEV).to(tdt).contiguous(), 32, N, sdt)
        assert rc == 0 and g.outside_intact()
        assert torch.equal(sim.cpu(), want), (dtype, e, (sim.cpu() != want).nonzero()[:5])


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("nq", [1, 7, 32])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_stream_random_unit_norm(dtype, nq):
    tdt, sdt = DTYPES[dtype]
    N = 1000
    gen = torch.Generator().manual_seed(7 + nq)
    fusion = _unit(torch.randn((nq, 256), generator=gen)).to(tdt)
    feats = _unit(torch.randn((N, 32, 256), generator=gen))
    away = -(torch.linalg.pinv(fusion.double()) @ torch.ones(nq, dtype=torch.float64)).float()             # <q, away> = -1 for every query
    anti = _unit(_unit(away) + 0.005 * torch.randn((N, 32, 256), generator=gen))                          # every row against every query
    for name, gal in (("random", feats), ("anti-aligned", anti)):
        gal = gal.to(tdt)
        rc, g, sim = _stream_raw(fusion.to(DEV), gal.to(DEV).contiguous(), nq, N, sdt)
        assert rc == 0 and g.outside_intact()
        q64, f64 = fusion.double().numpy(), gal.double().numpy()
        s = np.einsum("qk,njk->qnj", q64, f64)                                   # the rounded operands' scores, float64
        a = np.einsum("qk,njk->qnj", np.abs(q64), np.abs(f64))
        b = 2.0 * 256 * 2.0 ** -24 * a + 2.0 ** -23 * np.abs(s)                  # every row's own bound
        got = sim.cpu().numpy().astype(np.float64)
        lo, hi = (s - b).max(-1), (s + b).max(-1)
        jstar = s.argmax(-1)
        s_star, b_star = np.take_along_axis(s, jstar[..., None], -1)[..., 0], np.take_along_axis(b, jstar[..., None], -1)[..., 0]
        err = np.abs(got - s_star)
        print(f"[stream {dtype} nq={nq} {name}] max |sim - fp64| = {err.max():.3e}, worst error / bound = {(err / b_star).max():.3f}, max score {s_star.max():+.4f}")
        assert np.isfinite(got).all() and (got >= lo).all() and (got <= hi).all(), (name, dtype, nq)
        clear = (np.sort(s + b, -1)[..., -2] < s_star - b_star)                  # no other row within its own bound of the arg-max row
        assert (err[clear] <= b_star[clear]).all()
        if name == "anti-aligned":
            assert s_star.max() < -0.1                                            # negative maxima: a zero-initialised max would fail
            assert (got < 0).all()


def test_stream_refusals():
    lib = L.load()
    fusion = torch.zeros((33, 256), dtype=torch.float16, device=DEV)
    feats = torch.zeros((4, 32, 256), dtype=torch.float16, device=DEV)
    f32q, f32g = fusion.float(), feats.float()
    cases = {
        "nq=0": dict(nq=0), "nq=33": dict(nq=33), "E=128": dict(E_=128), "fp32": dict(dt=L.SPRC_F32, fusion=f32q, feats=f32g),
        "fp8": dict(dt=L.SPRC_FP8), "N=0": dict(N=0), "ld<N": dict(ld=3), "null fusion": dict(fusion=None), "null feats": dict(feats=None),
        "misaligned fusion": dict(ptr_shift=(8, 0)), "misaligned feats": dict(ptr_shift=(0, 2)),
    }
    for name, kw in cases.items():
        a = dict(fusion=fusion, feats=feats, nq=2, N=4, dt=L.SPRC_F16)
        a.update(kw)
        rc, g, _ = _stream_raw(a.pop("fusion"), a.pop("feats"), a.pop("nq"), a.pop("N"), a.pop("dt"), **a)
        assert rc != 0, name
        assert lib.sprc_last_error().decode(), name
        assert g.outside_intact(whole=True), name
    rc = lib.sprc_sim_max_stream(fusion.data_ptr(), feats.data_ptr(), None, 4, 2, 4, 256, L.SPRC_F16, None)
    assert rc != 0 and lib.sprc_last_error().decode()
    with pytest.raises(ValueError):
        E.search_topk(fusion[:1], feats, 0)
    with pytest.raises(ValueError):
        E.search_topk(fusion[:1], feats, 257)


@pytest.mark.parametrize("N", [1, 5, 64, 65, 4097, 20000])
def test_search_topk_is_single_level(N):
    """Every (nq, k, S): search_topk == E.topk / E.topk_wide on the stream kernel's own scores, bit for bit.  Image 0 is repeated at
    rows spread over the gallery (equal keys meet across segment boundaries: the lower index comes first) and query 0 points at it."""
    gen = torch.Generator(device=DEV).manual_seed(N)
    feats = _unit(torch.randn((N, 32, 256), generator=gen, device=DEV)).to(torch.float16)
    dup = sorted({(i * N) // 9 for i in range(9)} | {N - 1})
    feats[dup] = feats[0].clone()
    fusion = _unit(torch.randn((70, 256), generator=gen, device=DEV)).to(torch.float16)
    fusion[0] = feats[0, 3]
    for nq in (1, 3, 32, 33, 70):
        sim = E.sim_max_stream(fusion[:nq].contiguous(), feats)
        if N >= 64:
            assert int((sim[0] == sim[0, 0]).sum()) >= len(dup)
        for k in (1, 50, 64, 65, 200):
            wv, wi = E.topk(sim, k) if k <= 64 else E.topk_wide(sim, k)
            if nq == 1 and k >= len(dup) and N >= 64:
                assert wi[0, :len(dup)].tolist() == dup
            for S in (1, 2, 3, 7, None):
                v, i = E.search_topk(fusion[:nq].contiguous(), feats, k, S=S)
                assert torch.equal(i, wi), (N, nq, k, S)
                assert torch.equal(v.view(torch.int32), wv.view(torch.int32)), (N, nq, k, S)
    if N == 20000:
        assert E.search_segments(1, N)[1] > 1                                   # the automatic rule cuts this row


# ---- Searcher and the command line, end to end -------------------------------------------------------------------------------------
N_IMG, DEPTH = 14, 1
WORDS = ["make", "the", "dog", "bigger", "remove", "person", "add", "a", "red", "hat", "and", "two", "cats", "instead", "of", "one",
         "brighter", "background", "is", "more", "colour", "##ful", "##s", "##er", "left", "right"]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """~14 PNG files of assorted sizes, a synthetic vocabulary, two depth-1 checkpoints, and the fp16 store `search build` writes."""
    import sys
    from PIL import Image
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    from gen_preprocess_golden import synth_image
    from sprc_amd import search, synth
    from sprc_amd.config import get_config
    root = tmp_path_factory.mktemp("search_world")
    (root / "images" / "more").mkdir(parents=True)
    sizes = [(500, 375), (300, 600), (224, 224), (640, 200), (97, 301), (333, 333), (260, 190)]
    names = []
    for i in range(N_IMG):
        w, h = sizes[i % len(sizes)]
        arr = synth_image(w, h, 70 + i)
        name = f"item-{i:03d}"
        sub = "more" if i % 5 == 0 else "."
        if i == 4:                                            # one grayscale file
            Image.fromarray(arr[:, :, 0], mode="L").save(root / "images" / sub / f"{name}.png")
        else:
            Image.fromarray(arr).save(root / "images" / sub / f"{name}.png")
        names.append(name)
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + [".", ","]
    vocab += [f"tok{i}" for i in range(30522 - len(vocab))]
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    cfg = get_config("pretrain", vit_depth=DEPTH)
    for seed, fn in ((23, "ckpt.pt"), (24, "ckpt_other.pt")):
        torch.save({"Blip2QformerCirAlignPrompt": synth.make_state_dict(cfg, seed=seed), "epoch": 0}, root / fn)
    before = os.environ.get("SPRC_BERT_VOCAB")
    os.environ["SPRC_BERT_VOCAB"] = str(root / "vocab.txt")
    base = ["--model-path", str(root / "ckpt.pt"), "--dtype", "fp16", "--vit-depth", str(DEPTH)]
    built = search.main(["build", "--images", str(root / "images"), "--out", str(root / "store.safetensors"), "--feats-dtype", "fp16"] + base)
    assert built["images"] == N_IMG
    yield dict(root=root, names=names, base=base, store=str(root / "store.safetensors"), cfg=cfg)
    if before is None:
        os.environ.pop("SPRC_BERT_VOCAB", None)
    else:
        os.environ["SPRC_BERT_VOCAB"] = before


@pytest.fixture(scope="module")
def loaded(world):
    from sprc_amd.blip_validate import _load
    model, _ = _load("blip2_cir_align_prompt", "pretrain", str(world["root"] / "ckpt.pt"), "fp16", DEPTH)
    return model


def test_search_store_and_cli_forms(world, capsys):
    """The store holds fp16 feats and raw; a stored reference and the same image as a file give the same list; --json prints it."""
    from sprc_amd import search
    from sprc_amd.index import load_index
    (feats, raw), names, meta = load_index(world["store"], keep_feats_dtype=True)
    assert feats.dtype == torch.float16 and tuple(feats.shape) == (N_IMG, 32, 256) and meta["feats_dtype"] == "fp16"
    assert names == sorted(world["names"]) and raw is not None and raw.shape[0] == N_IMG
    q = ["query", "--index", world["store"], "--caption", "Make the dog bigger and add a red hat.", "-k", "5"] + world["base"]
    capsys.readouterr()
    by_name = search.main(q + ["--reference", "item-005"])
    lines = [l.split() for l in capsys.readouterr().out.splitlines() if l.strip() and l.split()[0].isdigit()]
    assert [(l[1], float(l[2])) for l in lines[-5:]] == [(n, pytest.approx(v, abs=1e-6)) for n, v in by_name]
    assert [l[0] for l in lines[-5:]] == ["1", "2", "3", "4", "5"]
    by_file = search.main(q + ["--reference-image", str(world["root"] / "images" / "more" / "item-005.png"), "--json"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert len(by_name) == 5 and by_file == by_name
    assert [(r["rank"], r["name"], r["score"]) for r in printed["results"]] == [(i + 1, n, v) for i, (n, v) in enumerate(by_file)]


def test_search_refuses_other_checkpoint_and_missing_raw(world):
    from sprc_amd import search
    q = ["query", "--index", world["store"], "--caption", "add a hat", "--reference", "item-001", "--dtype", "fp16", "--vit-depth", str(DEPTH)]
    with pytest.raises(ValueError, match="another checkpoint"):
        search.main(q + ["--model-path", str(world["root"] / "ckpt_other.pt")])
    bare = str(world["root"] / "bare.safetensors")
    search.main(["build", "--images", str(world["root"] / "images"), "--out", bare, "--keep-raw", "none", "--gpu-preprocess"] + world["base"])
    with pytest.raises(KeyError, match="no raw embeddings"):
        search.main(["query", "--index", bare, "--caption", "add a hat", "--reference", "item-001"] + world["base"])


def test_searcher_matches_the_existing_path(world, loaded, monkeypatch):
    """search_ids (no vocabulary) against model.similarity(rank_dtype="fp16") + E.topk on the same fusion vectors: scores inside the
    interval of the random-rows test at the returned ids; ids equal wherever the existing path's neighbouring scores are more than
    twice the bound apart; at most 10 % of the (query, position) pairs are exempt."""
    from sprc_amd import synth
    from sprc_amd.search import Searcher
    monkeypatch.delenv("SPRC_BERT_VOCAB", raising=False)
    loaded._tokenizer = None
    s = Searcher(loaded, world["store"])
    assert s.rank_dtype == torch.float16 and s.feats.dtype == torch.float16 and s.feats.is_cuda
    nq, k = 12, 10
    ids, mask, ref = synth.make_queries(nq, N_IMG, seed=5)
    refs = [s.names[int(r)] for r in ref]
    timings = {}
    vals, idx = s.search_ids(refs, ids, mask, k, timings=timings)
    assert tuple(vals.shape) == (nq, k) and idx.dtype == torch.int32 and set(timings) == {"reference_ms", "fuse_ms", "rank_ms"}
    # the existing path on the same fusion vectors
    fusion = loaded.fuse(s.reference_embeds(refs), ids.to(loaded.device), mask.to(loaded.device))
    loaded.rank_dtype = "fp16"
    sim = loaded.similarity(fusion, s.feats.float())
    wv, wi = E.topk(sim, k)
    q64, f64 = fusion.to(torch.float16).double().cpu().numpy(), s.feats.double().cpu().numpy()
    sc = np.einsum("qk,njk->qnj", q64, f64)
    b = 2.0 * 256 * 2.0 ** -24 * np.einsum("qk,njk->qnj", np.abs(q64), np.abs(f64)) + 2.0 ** -23 * np.abs(sc)
    lo, hi, bound = (sc - b).max(-1), (sc + b).max(-1), float(b.max())
    vals, idx, wv, wi = vals.cpu().numpy().astype(np.float64), idx.cpu().numpy(), wv.cpu().numpy().astype(np.float64), wi.cpu().numpy()
    rows = np.arange(nq)[:, None]
    assert (idx >= 0).all() and (vals >= lo[rows, idx]).all() and (vals <= hi[rows, idx]).all()
    gap_prev = np.concatenate([np.full((nq, 1), np.inf), wv[:, :-1] - wv[:, 1:]], axis=1)
    full = np.sort(sim.cpu().numpy().astype(np.float64), axis=1)[:, ::-1]                       # (position k - 1's next neighbour is rank k)
    gap_next = full[:, :k] - full[:, 1:k + 1]
    decided = (gap_prev > 2 * bound) & (gap_next > 2 * bound)
    exempt = 1.0 - decided.mean()
    print(f"[searcher] bound {bound:.3e}, smallest neighbour gap {min(gap_prev.min(), gap_next.min()):.3e}, exempt positions {exempt:.1%}, "
          f"max |score - existing| {np.abs(vals - wv).max():.3e}, timings {timings}")
    assert (idx[decided] == wi[decided]).all()
    assert exempt <= 0.10
    # captions through the vocabulary-free path agree with the names interface's shape: a mixed reference list
    img = synth.make_images(1, seed=9)[0]
    v2, i2 = s.search_ids([refs[0], img, world["root"] / "images" / "item-001.png"], ids[:3], mask[:3], 3)
    assert tuple(i2.shape) == (3, 3) and np.array_equal(i2[0].cpu().numpy(), idx[0, :3])
    with pytest.raises(KeyError):
        s.search_ids(["no-such-name"], ids[:1], mask[:1], 3)
