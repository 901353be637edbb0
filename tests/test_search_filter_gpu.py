"""Filtered index search on the GPU: the row-list score kernel (sprc_sim_max_stream_rows), E.search_topk(rows=, exclude=) and the
`sprc_amd.search` filters and edits end to end.

Every raw call of the kernel writes into a score buffer with ld_sim = M + 5 inside a sentinel-filled allocation (tests/_train_ref.py:
Guard) whose bits outside sim[q < nq, 0..M) are compared afterwards.  Bars:
  * exact data (integers in [-8, 8] x 2^-6: every product a multiple of 2^-12, every 256-term sum below 4, so fp32 accumulation is
    exact in any order): bit-equal to a float64 numpy evaluation at the listed rows and to sprc_sim_max_stream's columns `rows`;
  * random unit-norm rows: bit-equal to sprc_sim_max_stream's columns `rows` -- derived, not measured: an image's score is the same
    16-MFMA chain on the same operands in both kernels, whatever position of whatever list the image is reached through;
  * search_topk(rows=, exclude=): indices equal and values bit-equal to E.topk / E.topk_wide on the unfiltered kernel's scores with
    every column that is not listed, and the excluded one, set to -inf (index -1 wherever the value is -inf).
Out-of-range row values are not run here: the kernel's clamp is a defence, the interface is the validated list (host tests).
"""
import json
import os
import shutil
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
NEG = float("-inf")


def _rows_raw(fusion, feats, rows, nq, M, N, dt, ld_extra=5, E_=256, ld=None, ptr_shift=(0, 0)):
    """One raw sprc_sim_max_stream_rows call into a guarded buffer -> (rc, guard, logical sim view [nq, M])."""
    lib = L.load()
    ld = M + ld_extra if ld is None else ld
    g, sim = strided(max(nq, 1), max(M, 1), max(ld, max(M, 1)), device=DEV)
    g.seal()
    rc = lib.sprc_sim_max_stream_rows(None if fusion is None else fusion.data_ptr() + ptr_shift[0],
                                      None if feats is None else feats.data_ptr() + ptr_shift[1], None if rows is None else rows.data_ptr(),
                                      sim.data_ptr(), ld, nq, M, N, E_, dt, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, g, sim


def _grid():
    return E.STREAM_WG_PER_CU * L.load().sprc_stream_cus(None)


def _dev_rows(rows):
    return torch.as_tensor(np.asarray(rows), dtype=torch.int32).to(DEV).contiguous()


_EXACT = {}


def _exact_case(N):
    """(queries [32,256] fp32, gallery [N,32,256] fp32) holding integers in [-8, 8] x 2^-6, and a function rows -> float64 scores
    [32, len(rows)] (evaluated at the listed images only, in chunks: the long case's gallery is 12 000 images)."""
    if N not in _EXACT:
        rng = np.random.default_rng(1000 + N)
        q = rng.integers(-8, 9, size=(32, 256)).astype(np.float64) / 64.0
        f = rng.integers(-8, 9, size=(N, 32, 256), dtype=np.int8)
        _EXACT[N] = (torch.from_numpy(q.astype(np.float32)), torch.from_numpy(f).to(torch.float32) / 64.0, q, f)
    q32, f32, q, f = _EXACT[N]

    def ref(rows):
        rows = np.asarray(rows)
        out = np.empty((32, len(rows)))
        for s in range(0, len(rows), 2048):
            fr = f[rows[s:s + 2048]].astype(np.float64) / 64.0
            out[:, s:s + len(fr)] = (fr.reshape(-1, 256) @ q.T).reshape(len(fr), 32, 32).max(axis=1).T
        return out
    return q32, f32, ref


def _small_lists(N):
    back = lambda n: list(range(N - n, N))                                          # noqa: E731
    return {"first": [0], "last": [N - 1], "ends": [0, N - 1], "identity": list(range(N)), "every second": list(range(0, N, 2)),
            "P-1 from the back": back(P - 1), "P from the back": back(P), "P+1 from the back": back(P + 1), "2P+1 from the back": back(2 * P + 1),
            "descending": list(range(N - 1, -1, -3)), "repeated": [4, 7, 7, 7, 2, 4, N - 1, N - 1, 0, 7, 11]}


def _check_exact(dtype, N, lists):
    tdt, sdt = DTYPES[dtype]
    q32, f32, ref = _exact_case(N)
    feats = f32.to(DEV).to(tdt).contiguous()
    assert torch.equal(feats[:64].float().cpu(), f32[:64])                          # the operands are exact in both 16-bit formats
    for nq in (1, 2, 31, 32):
        fusion = q32[:nq].to(DEV).to(tdt).contiguous()
        plain = E.sim_max_stream(fusion, feats)                                     # the unfiltered kernel, [nq, N]
        for name, rows in lists.items():
            M = len(rows)
            rc, g, sim = _rows_raw(fusion, feats, _dev_rows(rows), nq, M, N, sdt)
            assert rc == 0, L.load().sprc_last_error()
            assert g.outside_intact(), (dtype, nq, name)
            got = sim.cpu().numpy()
            r64 = ref(rows)[:nq]
            want = r64.astype(np.float32)
            assert np.array_equal(want.astype(np.float64), r64)                     # the float64 scores are fp32 numbers
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (dtype, nq, name, np.abs(got - want).max())
            cols = plain[:, _dev_rows(rows).long()]
            assert torch.equal(sim.contiguous().view(torch.int32), cols.contiguous().view(torch.int32)), (dtype, nq, name)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rows_exact_small_lists(dtype):
    """29 images (3 P + 5): one-element lists, the identity, strides, lists of P - 1 .. 2 P + 1 rows from the back, a descending list
    and one with repeated rows (the kernel does not care about order)."""
    N = 3 * P + 5
    _check_exact(dtype, N, _small_lists(N))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rows_exact_long_list(dtype):
    """More trips than workgroups and not a multiple: every workgroup takes 2 or 3 trips and the last one is short; the list is two
    of every three rows of a gallery of ceil(1.5 M) images."""
    M = P * (2 * _grid() + 3) + 5
    N = -(-3 * M // 2)
    rows = [n for n in range(N) if n % 3 != 1][:M]
    assert len(rows) == M and rows[-1] < N
    _check_exact(dtype, N, {"two of three": rows})


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("nq", [1, 7, 32])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rows_random_unit_norm(dtype, nq):
    tdt, sdt = DTYPES[dtype]
    N, M = 1500, 1000
    gen = torch.Generator().manual_seed(11 + nq)
    fusion = _unit(torch.randn((nq, 256), generator=gen)).to(tdt).to(DEV).contiguous()
    feats = _unit(torch.randn((N, 32, 256), generator=gen)).to(tdt).to(DEV).contiguous()
    rows = torch.randperm(N, generator=gen)[:M].to(torch.int32).to(DEV).contiguous()                  # any order
    rc, g, sim = _rows_raw(fusion, feats, rows, nq, M, N, sdt)
    assert rc == 0 and g.outside_intact()
    cols = E.sim_max_stream(fusion, feats)[:, rows.long()]
    assert bool(torch.isfinite(sim).all())
    assert torch.equal(sim.contiguous().view(torch.int32), cols.contiguous().view(torch.int32)), (dtype, nq)
    out = E.sim_max_stream(fusion, feats, rows=rows)                                                  # the engine's wrapper, compact output
    assert tuple(out.shape) == (nq, M) and torch.equal(out.view(torch.int32), cols.contiguous().view(torch.int32))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_rows_layout_probes(dtype):
    """The one-hot construction of the plain kernel's layout probe (one 1 per image at feats[n = (j, c), j, 8 c + e], query slot
    (5 c + 3) % 32 = e_{8 c + e}) read through a permutation of the 1024 images: the 1.0 lands at the permuted position."""
    tdt, sdt = DTYPES[dtype]
    N = 32 * 32
    j, c = torch.arange(32).repeat_interleave(32), torch.arange(32).repeat(32)
    slot = (5 * torch.arange(32) + 3) % 32
    plain = torch.zeros((32, N))
    plain[slot[c], torch.arange(N)] = 1.0
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    want = plain[:, perm]
    rows = perm.to(torch.int32).to(DEV).contiguous()
    for e in range(8):
        feats = torch.zeros((N, 32, 256))
        feats[torch.arange(N), j, 8 * c + e] = 1.0
        fusion = torch.zeros((32, 256))
        fusion[slot, 8 * torch.arange(32) + e] = 1.0
        rc, g, sim = _rows_raw(fusion.to(DEV).to(tdt), feats.to(DEV).to(tdt).contiguous(), rows, 32, N, N, sdt)
        assert rc == 0 and g.outside_intact()
        assert torch.equal(sim.cpu(), want), (dtype, e, (sim.cpu() != want).nonzero()[:5])


def test_rows_refusals():
    lib = L.load()
    fusion = torch.zeros((33, 256), dtype=torch.float16, device=DEV)
    feats = torch.zeros((4, 32, 256), dtype=torch.float16, device=DEV)
    rows = _dev_rows([0, 2, 3])
    f32q, f32g = fusion.float(), feats.float()
    cases = {
        "null rows": dict(rows=None), "M=0": dict(M=0), "ld<M": dict(ld=2), "nq=0": dict(nq=0), "nq=33": dict(nq=33), "E=128": dict(E_=128),
        "fp32": dict(dt=L.SPRC_F32, fusion=f32q, feats=f32g), "fp8": dict(dt=L.SPRC_FP8), "N=0": dict(N=0), "null fusion": dict(fusion=None),
        "null feats": dict(feats=None), "misaligned fusion": dict(ptr_shift=(8, 0)), "misaligned feats": dict(ptr_shift=(0, 2)),
    }
    for name, kw in cases.items():
        a = dict(fusion=fusion, feats=feats, rows=rows, nq=2, M=3, N=4, dt=L.SPRC_F16)
        a.update(kw)
        rc, g, _ = _rows_raw(a.pop("fusion"), a.pop("feats"), a.pop("rows"), a.pop("nq"), a.pop("M"), a.pop("N"), a.pop("dt"), **a)
        assert rc != 0, name
        assert lib.sprc_last_error().decode(), name
        assert g.outside_intact(whole=True), name
    rc = lib.sprc_sim_max_stream_rows(fusion.data_ptr(), feats.data_ptr(), rows.data_ptr(), None, 3, 2, 3, 4, 256, L.SPRC_F16, None)
    assert rc != 0 and lib.sprc_last_error().decode()
    for k in (0, 257):
        with pytest.raises(ValueError):
            E.search_topk(fusion[:1], feats, k, rows=rows)
    with pytest.raises(ValueError):
        E.search_topk(fusion[:2], feats, 1, exclude=torch.tensor([1], dtype=torch.int32))                # one entry per query


# ---- search_topk(rows=, exclude=) ---------------------------------------------------------------------------------------------------
def _want(sim, rows, ex, k):
    """The parent's own functions on the unfiltered scores: unlisted columns and the excluded one at -inf, then the one-level top-k."""
    nq, N = sim.shape
    masked = torch.full_like(sim, NEG)
    if rows is None:
        masked.copy_(sim)
    else:
        masked[:, rows.long()] = sim[:, rows.long()]
    if ex is not None:
        q = torch.nonzero(ex >= 0).flatten()
        masked[q, ex[q].long()] = NEG
    wv, wi = E.topk(masked, k) if k <= 64 else E.topk_wide(masked, k)
    return wv, torch.where(torch.isneginf(wv), torch.full_like(wi, -1), wi)


@pytest.mark.parametrize("N", [5, 65, 4097, 20000])
def test_search_topk_rows_and_exclude(N):
    """Image 0 is repeated at rows spread over the gallery, inside and outside every list and across segment boundaries (equal keys:
    the lower gallery row comes first), and query 0 points at it; its exclusion takes the first of them out."""
    gen = torch.Generator(device=DEV).manual_seed(N)
    feats = _unit(torch.randn((N, 32, 256), generator=gen, device=DEV)).to(torch.float16)
    dup = sorted({(i * N) // 9 for i in range(9)} | {N - 1})
    feats[dup] = feats[0].clone()
    fusion = _unit(torch.randn((33, 256), generator=gen, device=DEV)).to(torch.float16)
    fusion[0] = feats[0, 3]
    cpu = torch.Generator().manual_seed(N)
    third = set(dup[::2][:max(N // 3, 1)])                                          # every other duplicate inside, the rest outside
    for n in torch.randperm(N, generator=cpu).tolist():
        if len(third) >= max(N // 3, 1):
            break
        if n not in dup:
            third.add(n)
    third = sorted(third)
    lists = {"one": [N - 1], "a third": third, "all but one": [n for n in range(N) if n != dup[1]], "all": list(range(N))}
    assert [len(r) for r in lists.values()] == [1, max(N // 3, 1), N - 1, N]
    ex_all = torch.randint(0, N, (33,), generator=cpu).to(torch.int32)
    ex_all[0] = 0                                                                   # query 0: the image it points at
    ex_all[1::4] = -1                                                               # every fourth query excludes nothing
    ex_all[2] = third[0]
    for nq in (1, 3, 32, 33):
        fq = fusion[:nq].contiguous()
        sim = E.sim_max_stream(fq, feats)
        ex = ex_all[:nq].to(DEV)
        for rows in lists.values():
            M = len(rows)
            assert all(b > a for a, b in zip(rows, rows[1:]))
            drows = _dev_rows(rows)
            for excl in (None, ex):
                for k in (1, 50, 65, 200):
                    wv, wi = _want(sim, drows, excl, k)
                    admissible = [n for n in dup if n in set(rows) and not (excl is not None and n == 0)]
                    lead = min(k, len(admissible))
                    if N >= 65:
                        assert wi[0, :lead].tolist() == admissible[:lead]          # the duplicates first, the lower gallery row first
                    for S in (1, 3, None):
                        v, i = E.search_topk(fq, feats, k, S=S, rows=drows, exclude=excl)
                        assert i.dtype == torch.int32 and tuple(i.shape) == (nq, k)
                        assert torch.equal(i, wi), (N, M, nq, k, S, excl is not None)
                        assert torch.equal(v.view(torch.int32), wv.view(torch.int32)), (N, M, nq, k, S, excl is not None)
                        short = min(k, M)
                        assert bool((i[:, short:] == -1).all()) and bool(torch.isneginf(v[:, short:]).all())
        for k in (1, 65):                                                           # exclusion alone: no list
            wv, wi = _want(sim, None, ex, k)
            for S in (1, 3, None):
                v, i = E.search_topk(fq, feats, k, S=S, exclude=ex)
                assert torch.equal(i, wi) and torch.equal(v.view(torch.int32), wv.view(torch.int32)), (N, nq, k, S)
    if N == 20000:
        assert E.search_segments(1, N // 3)[1] == 1 < E.search_segments(1, N - 1)[1]      # the rule segments by M, not by N


# ---- Searcher and the command line, end to end -------------------------------------------------------------------------------------
N_IMG, N_NEW, DEPTH = 14, 2, 1
WORDS = ["make", "the", "dog", "bigger", "remove", "person", "add", "a", "red", "hat", "and", "two", "cats", "instead", "of", "one",
         "brighter", "background", "is", "more", "colour", "##ful", "##s", "##er", "left", "right"]
CAPTION = "Make the dog bigger and add a red hat."


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """14 PNG files of assorted sizes (and two more in a directory of their own), a synthetic vocabulary, a depth-1 checkpoint, the
    fp16 store `search build` writes for the 14 and the one it writes for all 16."""
    import sys
    from PIL import Image
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    from gen_preprocess_golden import synth_image
    from sprc_amd import search, synth
    from sprc_amd.config import get_config
    root = tmp_path_factory.mktemp("search_filter_world")
    (root / "images" / "more").mkdir(parents=True)
    (root / "new").mkdir()
    sizes = [(500, 375), (300, 600), (224, 224), (640, 200), (97, 301), (333, 333), (260, 190)]
    names = []
    for i in range(N_IMG + N_NEW):
        w, h = sizes[i % len(sizes)]
        arr = synth_image(w, h, 70 + i)
        name = f"item-{i:03d}"
        where = root / "new" if i >= N_IMG else root / "images" / ("more" if i % 5 == 0 else ".")
        if i == 4:                                            # one grayscale file
            Image.fromarray(arr[:, :, 0], mode="L").save(where / f"{name}.png")
        else:
            Image.fromarray(arr).save(where / f"{name}.png")
        names.append(name)
    shutil.copytree(root / "images", root / "all")
    for f in (root / "new").iterdir():
        shutil.copy(f, root / "all" / f.name)
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(99)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"] + WORDS + [".", ","]
    vocab += [f"tok{i}" for i in range(30522 - len(vocab))]
    (root / "vocab.txt").write_text("\n".join(vocab) + "\n")
    cfg = get_config("pretrain", vit_depth=DEPTH)
    torch.save({"Blip2QformerCirAlignPrompt": synth.make_state_dict(cfg, seed=23), "epoch": 0}, root / "ckpt.pt")
    before = os.environ.get("SPRC_BERT_VOCAB")
    os.environ["SPRC_BERT_VOCAB"] = str(root / "vocab.txt")
    base = ["--model-path", str(root / "ckpt.pt"), "--dtype", "fp16", "--vit-depth", str(DEPTH)]
    for images, store, n in (("images", "store.safetensors", N_IMG), ("all", "store16.safetensors", N_IMG + N_NEW)):
        built = search.main(["build", "--images", str(root / images), "--out", str(root / store), "--feats-dtype", "fp16"] + base)
        assert built["images"] == n
    yield dict(root=root, names=names[:N_IMG], new=names[N_IMG:], base=base, store=str(root / "store.safetensors"),
               store16=str(root / "store16.safetensors"))
    if before is None:
        os.environ.pop("SPRC_BERT_VOCAB", None)
    else:
        os.environ["SPRC_BERT_VOCAB"] = before


@pytest.fixture(scope="module")
def loaded(world):
    from sprc_amd.blip_validate import _load
    model, _ = _load("blip2_cir_align_prompt", "pretrain", str(world["root"] / "ckpt.pt"), "fp16", DEPTH)
    return model


REFS = ["item-005", "item-011"]
CAPS = [CAPTION, "Remove the person and add two cats."]


def test_searcher_within_and_exclude(world, loaded):
    from sprc_amd.search import Searcher
    s = Searcher(loaded, world["store"])
    full = s.search(REFS, CAPS, k=N_IMG)
    assert all(len(h) == N_IMG for h in full)
    five = ["item-009", "item-002", "item-005", "item-013", "item-002", "item-007"]                    # one name twice: 5 names
    for within in (five, s.subset(five), s.subset(sorted(s.row_of[n] for n in set(five)))):
        got = s.search(REFS, CAPS, k=10, within=within)
        assert got == [[(n, v) for n, v in h if n in five] for h in full]                              # only those, in the unfiltered order
        assert all(len(h) == 5 for h in got)                                                           # k = 10 asked, 5 admissible
    assert s.search(REFS, CAPS, k=3, within=five) == [[(n, v) for n, v in h if n in five][:3] for h in full]
    # the reference leaves, everything else moves up
    got = s.search(REFS, CAPS, k=N_IMG, exclude_reference=True)
    assert got == [[(n, v) for n, v in h if n != r] for h, r in zip(full, REFS)] and all(len(h) == N_IMG - 1 for h in got)
    # a reference given as a file is no gallery name: nothing to leave out
    files = [world["root"] / "images" / "more" / "item-005.png", "item-011"]
    by_file = s.search(files, CAPS, k=N_IMG, exclude_reference=True)
    assert by_file[0] == s.search(files, CAPS, k=N_IMG)[0] and [n for n, _ in by_file[1]] == [n for n, _ in got[1]]
    out = ["item-000", full[0][0][0]]
    got = s.search(REFS, CAPS, k=N_IMG, exclude=out)
    assert got == [[(n, v) for n, v in h if n not in out] for h in full]
    got = s.search(REFS, CAPS, k=4, within=five, exclude=["item-002"], exclude_reference=True)
    assert got == [[(n, v) for n, v in h if n in five and n != "item-002" and n != r][:4] for h, r in zip(full, REFS)]
    for bad, err in ((dict(within=["item-001", "nope"]), KeyError), (dict(exclude=["nope"]), KeyError), (dict(within=[]), ValueError),
                     (dict(within=["item-001"], exclude=["item-001"]), ValueError), (dict(within=torch.tensor([3, 1])), ValueError),
                     (dict(within=torch.tensor([0, N_IMG])), ValueError)):
        with pytest.raises(err):
            s.search(REFS, CAPS, k=3, **bad)
    many = s.search(REFS * 20, CAPS * 20, k=10, within=five, exclude_reference=True)                   # 40 queries: blocks of 32
    want = [[(n, v) for n, v in h if n in five and n != r] for h, r in zip(full, REFS)]
    assert [[n for n, _ in h] for h in many] == [[n for n, _ in h] for h in want] * 20


def test_searcher_remove_and_add(world, loaded):
    from sprc_amd.search import Searcher
    s = Searcher(loaded, world["store"])
    full = s.search(REFS, CAPS, k=N_IMG)
    handle = s.subset(["item-003", "item-004", "item-008"])
    names_before = list(s.names)
    s.remove(["item-003"])
    assert s.names == names_before                                                                     # the numbering stays
    assert s.search(REFS, CAPS, k=N_IMG) == [[(n, v) for n, v in h if n != "item-003"] for h in full]
    assert s.search(REFS, CAPS, k=N_IMG, within=handle) == [[(n, v) for n, v in h if n in ("item-004", "item-008")] for h in full]
    with pytest.raises(KeyError):
        s.search(REFS, CAPS, k=3, within=["item-003"])
    with pytest.raises(KeyError):
        s.remove(["item-003"])
    with pytest.raises(ValueError):
        s.add(["item-004"], s.feats[:1])                                                               # a name of the gallery
    # two new files: the same results as a Searcher on a store built from all 16 files, ids mapped by name
    new_files = sorted((world["root"] / "new").iterdir())
    t = Searcher(loaded, world["store"])
    assert t.add_images(new_files) == world["new"] and t.names == world["names"] + world["new"] and t.feats.shape[0] == N_IMG + N_NEW
    u = Searcher(loaded, world["store16"])
    refs = REFS + [world["new"][0]]
    caps = CAPS + ["Add a red hat."]
    got, want = t.search(refs, caps, k=N_IMG + N_NEW), u.search(refs, caps, k=N_IMG + N_NEW)
    for g, w in zip(got, want):
        print("[add_images] max |score - built store| =", max(abs(a[1] - b[1]) for a, b in zip(g, w)))
        assert [n for n, _ in g] == [n for n, _ in w] and len(g) == N_IMG + N_NEW
        assert [v for _, v in g] == pytest.approx([v for _, v in w], abs=1e-3)
    vt, it = t.search_ids(refs, *_tokens(t, caps), 5, within=world["new"] + ["item-001"])
    vu, iu = u.search_ids(refs, *_tokens(u, caps), 5, within=world["new"] + ["item-001"])
    assert [[t.names[i] for i in r if i >= 0] for r in it.tolist()] == [[u.names[i] for i in r if i >= 0] for r in iu.tolist()]
    assert bool((it[:, 3:] == -1).all()) and bool(torch.isneginf(vt[:, 3:]).all())
    t.add(["copy-of-1"], t.feats[1:2].clone())                                                         # growth: a second append, no raw
    assert t.feats.shape[0] == N_IMG + N_NEW + 1 and t.search(REFS, CAPS, k=2, within=["copy-of-1", "item-001"])[0][0][0] == "item-001"


def _tokens(s, caps):
    tok = s.model.tokenizer([s.txt_processors["eval"](c) for c in caps], padding="max_length", truncation=True,
                            max_length=s.model.max_txt_len, return_tensors="pt")
    return tok.input_ids, tok.attention_mask


def test_cli_filters_and_edits(world, loaded, capsys, tmp_path):
    """`search add` / `search remove` on disk followed by `query` match the in-memory edits; the filter flags match the keywords."""
    from sprc_amd import search
    from sprc_amd.index import load_index
    from sprc_amd.search import Searcher
    s = Searcher(loaded, world["store"])
    q = ["query", "--caption", CAPTION, "--reference", "item-005", "-k", "8"] + world["base"]
    want = s.search(["item-005"], [CAPTION], k=8, within=[n for n in s.names if n.startswith("item-00")], exclude_reference=True)[0]
    got = search.main(q + ["--index", world["store"], "--within-glob", "item-00*", "--exclude-reference"])
    assert got == want and len(got) == 8 and all(n.startswith("item-00") and n != "item-005" for n, _ in got)
    listed = tmp_path / "names.txt"
    listed.write_text("item-012\n\nitem-003\nitem-005\n item-010 \n")
    want = s.search(["item-005"], [CAPTION], k=8, within=["item-012", "item-003", "item-005", "item-010"], exclude=["item-010"])[0]
    got = search.main(q + ["--index", world["store"], "--within-file", str(listed), "--exclude", "item-010", "--json"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert got == want and len(got) == 3 and [r["name"] for r in printed["results"]] == [n for n, _ in want]
    # add the two new files (the directory holds all 16: only the new stems are encoded), then drop one old row
    grown, edited = str(tmp_path / "grown.safetensors"), str(tmp_path / "edited.safetensors")
    before = Path(world["store"]).read_bytes()
    added = search.main(["add", "--index", world["store"], "--images", str(world["root"] / "all"), "--out", grown] + world["base"])
    assert added == {"index": grown, "added": N_NEW, "images": N_IMG + N_NEW} and Path(world["store"]).read_bytes() == before
    (f, raw), names, meta = load_index(grown, keep_feats_dtype=True)
    (f0, raw0), names0, meta0 = load_index(world["store"], keep_feats_dtype=True)
    assert names == names0 + world["new"] and meta == meta0 and f.dtype == torch.float16 and torch.equal(f[:N_IMG], f0)
    assert raw.shape[0] == N_IMG + N_NEW and torch.equal(raw[:N_IMG], raw0)
    removed = search.main(["remove", "--index", grown, "--names", "item-003", "--out", edited])
    assert removed == {"index": edited, "removed": 1, "images": N_IMG + N_NEW - 1}
    s.add_images(sorted((world["root"] / "new").iterdir()))
    s.remove(["item-003"])
    ref = world["new"][1]                                                                               # a new image as the stored reference
    want = s.search([ref], [CAPTION], k=16, exclude_reference=True)[0]
    got = search.main(["query", "--caption", CAPTION, "--reference", ref, "-k", "16", "--index", edited, "--exclude-reference"] + world["base"])
    assert [n for n, _ in got] == [n for n, _ in want] and len(got) == N_IMG + N_NEW - 2 and not {"item-003", ref} & {n for n, _ in got}
    assert [v for _, v in got] == pytest.approx([v for _, v in want], abs=1e-3)
