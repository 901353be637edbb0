"""CIRCO on the GPU: the multi-ground-truth metric kernel (sprc_ap_at_k) against sprc_rank_of, the numpy stable order and the
float64 formula; `python -m sprc_amd.blip_validate --dataset CIRCO` and `python -m sprc_amd.circo_test_submission` on a CIRCO
tree on disk (tests/_circo_tree.py) against an independent evaluation (PIL-exact transform + fp32 CPU oracle + this file's
numpy metric); the sharded evaluation on two gloo ranks sharing the GPU against the single-process harness."""
import ctypes as C
import importlib
import json
import os
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import _circo_tree as CT  # noqa: E402
import _dist_case as DC  # noqa: E402
from test_circo_cpu import KS, CircoRelative, brute_circo  # noqa: E402
from oracle import sprc_oracle as O  # noqa: E402
from oracle import preprocess_oracle as P  # noqa: E402
from sprc_amd import synth  # noqa: E402
from sprc_amd.config import get_config  # noqa: E402

DEV = "cuda:0"
DEPTH = 1
AP_TOL = 1e-12      # <= 32 correctly rounded fp64 terms, each <= 1, and one division: two orders of margin over 32 * 2^-53
MIN_GAP = 1e-4      # 16 x the 6e-6 the fp32 engine is documented to hold against the oracle


# ---- sprc_ap_at_k -----------------------------------------------------------------------------------------------------------------
def _scores(nq, N, extra, ties, seed):
    """-> (sim view [nq, N] with row stride N + extra, the columns beyond N filled with scores that would rank first)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    base = torch.rand((nq, N + extra), generator=g, device=DEV, dtype=torch.float32) * 2 - 1
    if ties:
        base = torch.round(base * 64) / 64                                   # at most 129 distinct values: rows full of ties
    if extra:
        base[:, N:] = 5.0
    return base[:, :N]


def _ground_truths(nq, N, G, seed):
    """[nq, G] int32: per row 0..min(G, N) distinct gallery indices in random slots, the other slots padding (-1, or an index >= N)"""
    rng = np.random.default_rng(seed)
    gt = np.full((nq, G), -1, dtype=np.int32)
    for q in range(nq):
        n = int(rng.integers(0, min(G, N) + 1)) if q % 5 else min(G, N)      # every fifth row full
        gt[q, rng.choice(G, size=n, replace=False)] = rng.choice(N, size=n, replace=False)
    if G > 1:
        gt[gt[:, -1] < 0, -1] = N + 3                                        # out of range = padding, like -1
    return gt


def _ap_float64(rank, ks):
    """the formula of include/sprc.h on exact ranks, in numpy float64"""
    ap = np.zeros((len(rank), len(ks)), dtype=np.float64)
    for q, row in enumerate(rank):
        r = np.sort(row[row >= 0]).astype(np.float64)
        for j, K in enumerate(ks):
            terms = (np.arange(len(r), dtype=np.float64) + 1.0) / (r + 1.0)
            ap[q, j] = terms[r < K].sum() / min(len(r), K) if len(r) else 0.0
    return ap


def _numpy_rank(sim_rows, gt_rows):
    """positions in the numpy stable order of fl32(1 - sim)"""
    out = np.full(gt_rows.shape, -1, dtype=np.int64)
    for q, (s, g) in enumerate(zip(sim_rows, gt_rows)):
        order = np.argsort(np.float32(1.0) - s, kind="stable")
        pos = np.empty(len(s), dtype=np.int64)
        pos[order] = np.arange(len(s))
        ok = (g >= 0) & (g < len(s))
        out[q, ok] = pos[g[ok]]
    return out


CASES = [(3, 1, 1, 0), (5, 1, 23, 3), (17, 37, 1, 0), (17, 37, 23, 5), (17, 37, 32, 0), (9, 2297, 1, 0), (64, 2297, 23, 7),
         (64, 2297, 32, 0), (40, 123403, 1, 0), (40, 123403, 32, 5), (800, 123403, 23, 0)]


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("nq,N,G,extra", CASES)
def test_ap_at_k_kernel(nq, N, G, extra, ties):
    from sprc_amd import engine as E
    sim = _scores(nq, N, extra, ties, seed=nq + N + G)
    assert sim.stride(0) == N + extra
    gt = _ground_truths(nq, N, G, seed=7 * nq + G)
    gt_t = torch.from_numpy(gt)
    ks = (5, 10, 25, 50)
    ap, rank = E.ap_at_k(sim, gt_t, ks)
    ap2, rank2 = E.ap_at_k(sim, gt_t, ks)
    torch.cuda.synchronize()
    assert ap.dtype == torch.float64 and ap.shape == (nq, 4) and rank.dtype == torch.int32 and rank.shape == (nq, G)
    assert torch.equal(ap.view(torch.int64), ap2.view(torch.int64)) and torch.equal(rank, rank2)          # the same bits, run to run
    rank_np = rank.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(rank_np, E.rank_of(sim, gt_t).cpu().numpy())
    rows = np.arange(nq) if nq * N <= 4_000_000 else np.unique(np.linspace(0, nq - 1, 24).astype(np.int64))
    np.testing.assert_array_equal(rank_np[rows], _numpy_rank(sim[torch.from_numpy(rows).to(DEV)].cpu().numpy(), gt[rows]))
    assert ((rank_np >= 0) == ((gt >= 0) & (gt < N))).all()
    got, want = ap.cpu().numpy(), _ap_float64(rank_np, ks)
    err = float(np.abs(got - want).max())
    print(f"ap_at_k nq={nq} N={N} G={G} ld={N + extra} ties={ties}: max |ap - float64 formula| = {err:.3e}")
    assert err <= AP_TOL
    assert (got[((gt >= 0) & (gt < N)).sum(1) == 0] == 0.0).all()                                          # no ground truth -> AP 0
    # other K lists: a single K, eight of them, K beyond the gallery
    for ks2 in ((1,), (1, 2, 3, 7, 50, 64, 1000, 200000)):
        ap3, _ = E.ap_at_k(sim, gt_t, ks2)
        assert float(np.abs(ap3.cpu().numpy() - _ap_float64(rank_np, ks2)).max()) <= AP_TOL


def test_ap_at_k_hand_worked_and_optional_rank():
    """ranks {0, 2, 5} with G = 3: AP@5 = (1/1 + 2/3) / 3, AP@10 = (1/1 + 2/3 + 3/6) / 3; `rank` may be NULL."""
    from sprc_amd import _lib as L
    lib = L.load()
    sim = torch.tensor([[0.9, 0.1, 0.7, 0.8, 0.6, 0.65, 0.2, 0.3]], device=DEV)          # order: 0 3 2 5 4 7 6 1
    gt = torch.tensor([[7, 0, -1, 2]], dtype=torch.int32, device=DEV)                    # ranks 5, 0, (padding), 2
    ap = torch.empty((1, 2), dtype=torch.float64, device=DEV)
    ks = (C.c_int32 * 2)(5, 10)
    st = torch.cuda.current_stream().cuda_stream
    L.check(lib.sprc_ap_at_k(sim.data_ptr(), 8, gt.data_ptr(), 1, 8, 4, ks, 2, ap.data_ptr(), None, st), "sprc_ap_at_k")
    torch.cuda.synchronize()
    assert ap.cpu().numpy()[0] == pytest.approx([(1 / 1 + 2 / 3) / 3, (1 / 1 + 2 / 3 + 3 / 6) / 3], abs=AP_TOL)


def test_ap_at_k_refuses_bad_arguments():
    from sprc_amd import _lib as L
    lib = L.load()
    sim = torch.zeros((2, 40), device=DEV)
    gt = (torch.arange(66, dtype=torch.int32, device=DEV) % 40).reshape(2, 33)       # distinct within the 23 entries of a row
    ap = torch.zeros((2, 9), dtype=torch.float64, device=DEV)
    ks = (C.c_int32 * 9)(*range(1, 10))
    good = dict(sim=sim.data_ptr(), ld=40, gt=gt.data_ptr(), nq=2, N=40, G=23, ks=ks, nk=4, ap=ap.data_ptr(), rank=None)

    def call(**over):
        a = {**good, **over}
        return lib.sprc_ap_at_k(a["sim"], a["ld"], a["gt"], a["nq"], a["N"], a["G"], a["ks"], a["nk"], a["ap"], a["rank"], None)

    for over, word in ((dict(G=33), b"G=33"), (dict(G=0), b"G=0"), (dict(nk=9), b"nk=9"), (dict(nk=0), b"nk=0"), (dict(sim=None), b"null pointer"),
                       (dict(gt=None), b"null pointer"), (dict(ks=None), b"null pointer"), (dict(ap=None), b"null pointer"),
                       (dict(ld=39), b"bad shape"), (dict(nq=0), b"bad shape"), (dict(ks=(C.c_int32 * 4)(5, 0, 25, 50)), b"must be >= 1")):
        assert call(**over) == -1, over                                      # SPRC_EINVAL
        assert word in lib.sprc_last_error(), (over, lib.sprc_last_error())
    with pytest.raises(L.SprcError, match="G=33"):
        L.check(call(G=33), "sprc_ap_at_k")
    assert call() == 0
    torch.cuda.synchronize()


# ---- the entry points on a CIRCO tree on disk ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    root = tmp_path_factory.mktemp("sprc_circo")
    tree = CT.build_circo_tree(root / "CIRCO")
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + CT.WORDS + [".", ","]
    vocab += [f"tok{i}" for i in range(30522 - len(vocab))]
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    cfg = get_config("pretrain", vit_depth=DEPTH)
    sd = synth.make_state_dict(cfg, seed=17)
    torch.save({"Blip2QformerCirAlignPrompt": sd, "epoch": 0}, root / "ckpt.pt")
    torch.save({"Blip2QformerCirAlignPrompt": synth.make_state_dict(cfg, seed=18), "epoch": 0}, root / "ckpt_other.pt")
    os.environ["SPRC_DATA_ROOT"], os.environ["SPRC_BERT_VOCAB"] = str(root), str(root / "vocab.txt")
    import sprc_amd.data_utils as du
    importlib.reload(du)                                   # base_path is read at import
    return dict(root=root, tree=tree, cfg=cfg, sd=sd, names=[str(i) for i in tree["ids"]])


def _oracle_scores(world, annotations):
    """independent scores: PIL-exact transform (oracle restatement) + fp32 CPU oracle"""
    from sprc_amd.processors import BlipCaptionProcessor
    from sprc_amd.tokenizer import BertWordPieceTokenizer
    cfg, sd, names = world["cfg"], world["sd"], world["names"]
    images = torch.from_numpy(np.stack([P.targetpad_transform(world["tree"]["arrays"][n]) for n in names]))
    proc, tok = BlipCaptionProcessor(), BertWordPieceTokenizer()
    t = tok([proc(a["relative_caption"]) for a in annotations], padding="max_length", truncation=True, max_length=32, return_tensors="pt")
    n2i = {n: i for i, n in enumerate(names)}
    ref = torch.tensor([n2i[str(a["reference_img_id"])] for a in annotations])
    with torch.no_grad():
        feats, raw = O.extract_target_features(sd, cfg, images)
        return O.inference(sd, cfg, raw[ref], feats, t.input_ids, t.attention_mask).numpy()


def test_blip_validate_circo_on_disk(world, tmp_path, capsys):
    """The seeds of tests/_circo_tree.py (QUERY_SEEDS) were chosen with the oracle alone, on the CPU: candidate seeds 0, 1, 2, ... in
    order, a seed kept when the 24 oracle scores of its query lie more than 1.2e-4 apart.  The bound asserted here is the one that
    makes the comparison meaningful: neighbouring oracle scores more than 1e-4 apart, the fp32 engine within 6e-6 of the oracle,
    hence identical ranks and mAP / recall equal to the last bit of the float64 means."""
    from sprc_amd import blip_validate as bv
    val = world["tree"]["val"]
    sim = _oracle_scores(world, val)
    gaps = np.diff(np.sort(sim.astype(np.float64), axis=1), axis=1)
    print(f"oracle scores: smallest gap between neighbours in a row = {gaps.min():.3e}")
    assert gaps.min() > MIN_GAP
    n2i = {n: i for i, n in enumerate(world["names"])}
    gt_lists = [list(dict.fromkeys(n2i[str(g)] for g in a["gt_img_ids"])) for a in val]
    want, _ = brute_circo(sim, gt_lists, [n2i[str(a["target_img_id"])] for a in val])
    args = ["--dataset", "CIRCO", "--model-path", str(world["root"] / "ckpt.pt"), "--dtype", "fp32", "--vit-depth", str(DEPTH)]
    capsys.readouterr()
    out = bv.main(args)                                                     # default path: <data root>/CIRCO
    assert json.loads(capsys.readouterr().out.split("Compute CIRCO validation metrics")[-1].strip()) == out
    assert set(out) == set(want) == {f"circo_{m}_at{k}" for m in ("map", "recall") for k in KS}
    for key in want:
        print(f"{key}: engine {out[key]!r} independent {want[key]!r}")
        assert out[key] == pytest.approx(want[key], abs=1e-9)
    assert 0 < out["circo_map_at5"] < 100                                   # (neither trivial end of the scale)
    args += ["--circo-path", str(world["root"] / "CIRCO")]
    assert bv.main(args) == out
    # GPU image transform (decode-only thread loader over the dict items): bit-identical pixels -> the same dict
    assert bv.main(args + ["--gpu-preprocess"]) == out
    # feature store: written once, reloaded, refused for another checkpoint
    cache = tmp_path / "index"
    assert bv.main(args + ["--index-cache", str(cache)]) == out
    assert len(list(cache.glob("circo-val-*.safetensors"))) == 1
    capsys.readouterr()
    assert bv.main(args + ["--index-cache", str(cache)]) == out
    assert "loaded 24 gallery rows" in capsys.readouterr().out
    other = bv.main(["--dataset", "CIRCO", "--model-path", str(world["root"] / "ckpt_other.pt"), "--dtype", "fp32", "--vit-depth", str(DEPTH),
                     "--index-cache", str(cache)])
    assert len(list(cache.glob("*.safetensors"))) == 2 and other != out     # its own store, its own numbers
    # the store keeps raw embeddings of the reference images only
    from sprc_amd.harness import RawStore
    from sprc_amd.index import load_index
    (_, raw), names, _ = load_index(sorted(cache.glob("*.safetensors"))[0])
    assert isinstance(raw, RawStore) and names == world["names"]
    assert {names[i] for i in raw.rows} == {str(a["reference_img_id"]) for a in val} and raw.kept < len(names)


def test_blip_validate_circo_reuse_reference_kv(world):
    """--reuse-reference-kv on the 16-bit engine: precomputed K|V of the reference images, looked up by id."""
    from sprc_amd import blip_validate as bv
    args = ["--dataset", "CIRCO", "--model-path", str(world["root"] / "ckpt.pt"), "--dtype", "fp16", "--vit-depth", str(DEPTH)]
    plain, reuse = bv.main(args), bv.main(args + ["--reuse-reference-kv"])
    assert set(plain) == set(reuse) and all(0.0 <= v <= 100.0 for v in reuse.values())
    assert reuse["circo_recall_at50"] == plain["circo_recall_at50"] == 100.0          # 24 images: every target is inside the top 50


def test_circo_test_submission_on_disk(world):
    from sprc_amd import circo_test_submission as cts
    cts.main(["--model-path", str(world["root"] / "ckpt.pt"), "--dtype", "fp32", "--vit-depth", str(DEPTH), "--gpu-preprocess"])
    sub = json.loads((world["root"] / "submission" / "CIRCO" / "circo_test_submission_blip2_cir_align_prompt.json").read_text())
    test = world["tree"]["test"]
    sim = _oracle_scores(world, test)
    assert np.diff(np.sort(sim.astype(np.float64), axis=1), axis=1).min() > MIN_GAP
    order = O.rank_stable(sim)
    names = np.asarray(world["names"])
    assert sub == {str(a["id"]): names[order[q, :50]].tolist() for q, a in enumerate(test)}
    assert all(len(v) == CT.N_IMG for v in sub.values())                    # the whole small gallery, the reference image included


# ---- sharded against single-process --------------------------------------------------------------------------------------------------
def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(torch.device(DEV))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from sprc_amd import dist_eval as DE
    from test_dist_gpu import _model
    case = DC.build(0)
    model = _model(case)
    gallery = DC.Gallery(case["images"])
    metrics = DE.compute_circo_val_metrics_sharded(CircoRelative(case), gallery, model, DC.TXT, num_workers=0, gallery_batch_size=16)
    top = DE.generate_circo_test_dicts_sharded(CircoRelative(case, test=True), gallery, model, DC.TXT, num_workers=0, gallery_batch_size=16)
    torch.cuda.synchronize()
    out[rank] = dict(metrics=metrics, top=top)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_the_single_process_circo_harness():
    from sprc_amd import harness as H
    from test_dist_gpu import _free_port, _model
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
        res = {r: dict(out[r]) for r in range(2)}
    case = DC.build(0)
    model = _model(case)
    rel = CircoRelative(case)
    (feats, raw), names = H.extract_index_blip_features(DC.Gallery(case["images"]), model, batch_size=16, num_workers=0,
                                                        keep_raw=H.circo_reference_ids(rel))
    assert isinstance(raw, H.RawStore) and raw.kept < len(names)
    want = H.compute_circo_val_metrics(rel, model, (feats, raw), names, DC.TXT)
    want_top = H.generate_circo_test_dicts(CircoRelative(case, test=True), model, (feats, raw), names, DC.TXT)
    assert len(names) > 50 and all(len(v) == 50 for v in want_top.values())
    for r in range(2):
        assert res[r]["metrics"] == want and res[r]["top"] == want_top
