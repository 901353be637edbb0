"""Per-query filters of the index search on the GPU: the admit-mask score kernel (sprc_sim_max_stream_admit),
E.search_topk(rows=, admit=), `Searcher.search(within_each=, exclude_each=)` and the `batch` command end to end.

Every raw call of the kernel writes into a score buffer with ld_sim = M + 5 inside a sentinel-filled allocation (tests/_train_ref.py:
Guard) whose bits outside sim[q < nq, 0..M) are compared afterwards.  Bars:
  * exact data (integers in [-8, 8] x 2^-6: every product a multiple of 2^-12, every 256-term sum below 4, so fp32 accumulation is
    exact in any order): where admitted bit-equal to a float64 numpy evaluation at the listed rows and to sprc_sim_max_stream's
    columns `rows`, -inf everywhere else;
  * random unit-norm rows: admitted entries bit-equal to sprc_sim_max_stream's columns `rows` -- derived, not measured: an admitted
    score is the same 16-MFMA chain on the same operands as in the plain kernel, whatever list position and admit word it is
    reached through -- and the rest -inf;
  * search_topk(rows=, admit=): indices equal and values bit-equal to E.topk / E.topk_wide on the unfiltered kernel's scores with
    every (q, n) that is not admitted, and the excluded one, set to -inf (index -1 wherever the value is -inf);
  * Searcher / batch: every query's answer equals the single-query answer with that query's filter, names and scores.
"""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _search_world as W  # noqa: E402
from _train_ref import strided  # noqa: E402
from sprc_amd import _lib as L  # noqa: E402
from sprc_amd import engine as E  # noqa: E402

DEV = "cuda:0"
DTYPES = {"fp16": (torch.float16, L.SPRC_F16), "bf16": (torch.bfloat16, L.SPRC_BF16)}
P = E.STREAM_P
NEG = float("-inf")
NEG_BITS = np.float32(NEG).view(np.uint32)


def _admit_raw(fusion, feats, rows, admit, nq, M, N, dt, ld_extra=5, E_=256, ld=None, ptr_shift=(0, 0)):
    """One raw sprc_sim_max_stream_admit call into a guarded buffer -> (rc, guard, logical sim view [nq, M])."""
    lib = L.load()
    ld = M + ld_extra if ld is None else ld
    g, sim = strided(max(nq, 1), max(M, 1), max(ld, max(M, 1)), device=DEV)
    g.seal()
    rc = lib.sprc_sim_max_stream_admit(None if fusion is None else fusion.data_ptr() + ptr_shift[0],
                                       None if feats is None else feats.data_ptr() + ptr_shift[1], None if rows is None else rows.data_ptr(),
                                       None if admit is None else admit.data_ptr(), sim.data_ptr(), ld, nq, M, N, E_, dt,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, g, sim


def _grid():
    return E.STREAM_WG_PER_CU * L.load().sprc_stream_cus(None)


def _dev_i32(a):
    return torch.as_tensor(np.asarray(a)).to(torch.int32).to(DEV).contiguous()


def _dev_words(words):
    return torch.from_numpy(np.asarray(words, dtype=np.uint32).view(np.int32).copy()).to(DEV).contiguous()


def _patterns(M, nq, seed):
    """The five admit patterns of a list of M positions (uint32 [M] each)."""
    rng = np.random.default_rng(seed)
    rnd = rng.integers(0, 2 ** 32, size=M, dtype=np.uint64).astype(np.uint32)          # neighbouring positions get different words
    high = np.uint32((0xFFFFFFFF << nq) & 0xFFFFFFFF)
    return {"ones": np.full(M, 0xFFFFFFFF, dtype=np.uint32), "zero": np.zeros(M, dtype=np.uint32),
            "walking bit": (np.uint32(1) << (np.arange(M, dtype=np.uint32) % 32)).astype(np.uint32), "random": rnd,
            "random, bits >= nq set": rng.integers(0, 2 ** 32, size=M, dtype=np.uint64).astype(np.uint32) | high}


def _small_lists(N):
    back = lambda n: list(range(N - n, N))                                          # noqa: E731
    return {"first": [0], "last": [N - 1], "ends": [0, N - 1], "identity": list(range(N)), "every second": list(range(0, N, 2)),
            "P-1 from the back": back(P - 1), "P from the back": back(P), "P+1 from the back": back(P + 1), "2P+1 from the back": back(2 * P + 1),
            "descending": list(range(N - 1, -1, -3)), "repeated": [4, 7, 7, 7, 2, 4, N - 1, N - 1, 0, 7, 11]}


def _check_exact(dtype, N, lists, patterns):
    tdt, sdt = DTYPES[dtype]
    q32, f8, ref = W.exact_case(N)
    feats = (f8.to(DEV).to(torch.float32) / 64.0).to(tdt).contiguous()
    assert torch.equal(feats[:64].float().cpu(), f8[:64].float() / 64.0)            # the operands are exact in both 16-bit formats
    for nq in (1, 2, 31, 32):
        fusion = q32[:nq].to(DEV).to(tdt).contiguous()
        plain = E.sim_max_stream(fusion, feats)                                     # the unfiltered kernel, [nq, N]
        for name, rows in lists.items():
            M = len(rows)
            r64 = ref(rows)[:nq]
            want = r64.astype(np.float32)
            assert np.array_equal(want.astype(np.float64), r64)                     # the float64 scores are fp32 numbers
            drows = _dev_i32(rows)
            cols = plain[:, drows.long()].cpu().numpy().view(np.uint32)
            for pname, words in _patterns(M, nq, 7 * M + nq).items():
                if pname not in patterns:
                    continue
                rc, g, sim = _admit_raw(fusion, feats, drows, _dev_words(words), nq, M, N, sdt)
                assert rc == 0, L.load().sprc_last_error()
                assert g.outside_intact(), (dtype, nq, name, pname)
                got = sim.cpu().numpy().view(np.uint32)
                adm = W.admitted(words, nq)
                assert np.array_equal(got, np.where(adm, want.view(np.uint32), NEG_BITS)), (dtype, nq, name, pname)
                assert np.array_equal(got, np.where(adm, cols, NEG_BITS)), (dtype, nq, name, pname)
                if pname == "zero":
                    assert bool(torch.isneginf(sim).all())


ALL_PATTERNS = ("ones", "zero", "walking bit", "random", "random, bits >= nq set")


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_admit_exact_small_lists(dtype):
    """29 images (3 P + 5): one-element lists, the identity, strides, lists of P - 1 .. 2 P + 1 rows from the back, a descending list
    and one with repeated rows, each under the five admit patterns."""
    N = 3 * P + 5
    _check_exact(dtype, N, _small_lists(N), ALL_PATTERNS)


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_admit_exact_long_list(dtype):
    """More trips than workgroups and not a multiple: every workgroup takes 2 or 3 trips and the last one is short, so the admit word
    fetched a trip ahead is used in every loop trip and in the peeled tail; two of every three rows of ceil(1.5 M) images."""
    M = P * (2 * _grid() + 3) + 5
    N = -(-3 * M // 2)
    rows = [n for n in range(N) if n % 3 != 1][:M]
    assert len(rows) == M and rows[-1] < N
    _check_exact(dtype, N, {"two of three": rows}, ("random", "random, bits >= nq set"))


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("nq", [1, 7, 32])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_admit_random_unit_norm(dtype, nq):
    tdt, sdt = DTYPES[dtype]
    N, M = 1500, 1000
    gen = torch.Generator().manual_seed(23 + nq)
    fusion = _unit(torch.randn((nq, 256), generator=gen)).to(tdt).to(DEV).contiguous()
    feats = _unit(torch.randn((N, 32, 256), generator=gen)).to(tdt).to(DEV).contiguous()
    rows = torch.randperm(N, generator=gen)[:M].to(torch.int32).to(DEV).contiguous()                  # any order
    words = _patterns(M, nq, 31 + nq)["random"]
    admit = _dev_words(words)
    rc, g, sim = _admit_raw(fusion, feats, rows, admit, nq, M, N, sdt)
    assert rc == 0 and g.outside_intact()
    cols = E.sim_max_stream(fusion, feats)[:, rows.long()]
    assert bool(torch.isfinite(cols).all())
    adm = torch.from_numpy(W.admitted(words, nq)).to(DEV)
    assert 0 < int(adm.sum()) < adm.numel()
    want = torch.where(adm, cols, torch.full_like(cols, NEG)).contiguous()
    assert torch.equal(sim.contiguous().view(torch.int32), want.view(torch.int32)), (dtype, nq)
    out = E.sim_max_stream(fusion, feats, rows=rows, admit=admit.view(1, M))                          # the engine's wrapper, compact output
    assert tuple(out.shape) == (nq, M) and torch.equal(out.view(torch.int32), want.view(torch.int32))


def test_admit_refusals():
    lib = L.load()
    fusion = torch.zeros((33, 256), dtype=torch.float16, device=DEV)
    feats = torch.zeros((4, 32, 256), dtype=torch.float16, device=DEV)
    rows, admit = _dev_i32([0, 2, 3]), _dev_words([3, 1, 2])
    f32q, f32g = fusion.float(), feats.float()
    cases = {
        "null admit": dict(admit=None), "null rows": dict(rows=None), "M=0": dict(M=0), "ld<M": dict(ld=2), "nq=0": dict(nq=0),
        "nq=33": dict(nq=33), "E=128": dict(E_=128), "fp32": dict(dt=L.SPRC_F32, fusion=f32q, feats=f32g), "fp8": dict(dt=L.SPRC_FP8),
        "N=0": dict(N=0), "null fusion": dict(fusion=None), "null feats": dict(feats=None), "misaligned fusion": dict(ptr_shift=(8, 0)),
        "misaligned feats": dict(ptr_shift=(0, 2)),
    }
    for name, kw in cases.items():
        a = dict(fusion=fusion, feats=feats, rows=rows, admit=admit, nq=2, M=3, N=4, dt=L.SPRC_F16)
        a.update(kw)
        rc, g, _ = _admit_raw(a.pop("fusion"), a.pop("feats"), a.pop("rows"), a.pop("admit"), a.pop("nq"), a.pop("M"), a.pop("N"), a.pop("dt"), **a)
        assert rc != 0, name
        assert lib.sprc_last_error().decode(), name
        assert g.outside_intact(whole=True), name
    rc = lib.sprc_sim_max_stream_admit(fusion.data_ptr(), feats.data_ptr(), rows.data_ptr(), admit.data_ptr(), None, 3, 2, 3, 4, 256, L.SPRC_F16, None)
    assert rc != 0 and lib.sprc_last_error().decode()
    good = admit.view(1, 3)
    with pytest.raises(ValueError):
        E.search_topk(fusion[:2], feats, 1, admit=good)                                               # admit requires rows
    with pytest.raises(ValueError):
        E.sim_max_stream(fusion[:2], feats, admit=good)
    for bad in (admit, admit.view(3, 1), torch.zeros((2, 3), dtype=torch.int32, device=DEV), torch.zeros((1, 4), dtype=torch.int32, device=DEV),
                good.long(), torch.zeros((1, 6), dtype=torch.int32, device=DEV)[:, ::2], good.cpu()):
        with pytest.raises(ValueError):
            E.search_topk(fusion[:2], feats, 1, rows=rows, admit=bad)
    with pytest.raises(ValueError):
        E.search_topk(fusion, feats, 1, rows=rows, admit=good)                                        # 33 queries: two rows of words


# ---- search_topk(rows=, admit=) -----------------------------------------------------------------------------------------------------
def _want(sim, member, ex, k):
    """The parent's own functions on the unfiltered scores: every (q, n) that is not admitted and the excluded one at -inf, then the
    one-level top-k."""
    masked = torch.where(member, sim, torch.full_like(sim, NEG))
    if ex is not None:
        q = torch.nonzero(ex >= 0).flatten()
        masked[q, ex[q].long()] = NEG
    wv, wi = E.topk(masked, k) if k <= 64 else E.topk_wide(masked, k)
    return wv, torch.where(torch.isneginf(wv), torch.full_like(wi, -1), wi)


@pytest.mark.parametrize("N", [5, 65, 4097, 20000])
def test_search_topk_rows_and_admit(N):
    """Image 0 is repeated at rows spread over the gallery, inside and outside every list and across segment boundaries (equal keys:
    the lower gallery row comes first), and query 0 points at it.  The four lists -- one row, a third of the rows, all but one, all --
    go to the queries in rotation, so one call mixes queries that admit one image (fewer than k) with queries that admit all."""
    gen = torch.Generator(device=DEV).manual_seed(N + 1)
    feats = _unit(torch.randn((N, 32, 256), generator=gen, device=DEV)).to(torch.float16)
    dup = sorted({(i * N) // 9 for i in range(9)} | {N - 1})
    feats[dup] = feats[0].clone()
    fusion = _unit(torch.randn((70, 256), generator=gen, device=DEV)).to(torch.float16)
    fusion[0] = feats[0, 3]
    fusion[1::5] = feats[0, 3]                                                      # more queries whose best images are the duplicates
    fusion[3] = feats[0, 3]
    cpu = torch.Generator().manual_seed(N + 1)
    third = set(dup[::2][:max(N // 3, 1)])                                          # every other duplicate inside, the rest outside
    for n in torch.randperm(N, generator=cpu).tolist():
        if len(third) >= max(N // 3, 1):
            break
        if n not in dup:
            third.add(n)
    lists = [[N - 1], sorted(third), [n for n in range(N) if n != dup[1]], list(range(N))]
    assert [len(r) for r in lists] == [1, max(N // 3, 1), N - 1, N]
    ex_all = torch.randint(0, N, (70,), generator=cpu).to(torch.int32)
    ex_all[1] = 0                                                                   # query 1 (a third of the rows): the image it points at
    ex_all[2::4] = -1                                                               # every fourth query excludes nothing
    for nq in (1, 3, 32, 33, 70):
        fq = fusion[:nq].contiguous()
        sim = E.sim_max_stream(fq, feats)
        member_all = np.zeros((nq, N), dtype=bool)
        for q in range(nq):
            member_all[q, lists[(q + (nq == 1)) % 4]] = True                        # (a single query takes the second list, not one row)
        if nq == 3:
            member_all[2] = False
            member_all[2, lists[0]] = True                                          # one, a third, one: a union that is a proper subset
        rows = np.flatnonzero(member_all.any(axis=0))
        M = len(rows)
        assert M == (N if nq >= 4 else max(N // 3, 1) + (nq == 3 and N - 1 not in third))
        drows = _dev_i32(rows)
        admit = W.admit_words(member_all[:, rows]).to(DEV)
        assert tuple(admit.shape) == (-(-nq // 32), M)
        member = torch.from_numpy(member_all).to(DEV)
        ex = ex_all[:nq].to(DEV)
        for excl in (None, ex):
            for k in (1, 50, 65, 200):
                wv, wi = _want(sim, member, excl, k)
                if nq >= 4 and N >= 65 and excl is None:
                    assert wi[0, 0].item() == N - 1 and wi[0, 1:].eq(-1).all()      # query 0 admits one image: fewer than k
                    lead = min(k, len(dup))
                    assert wi[3, :lead].tolist() == dup[:lead]                      # query 3 admits all: the duplicates, lower row first
                for S in (1, 3, None):
                    v, i = E.search_topk(fq, feats, k, S=S, rows=drows, exclude=excl, admit=admit)
                    assert i.dtype == torch.int32 and tuple(i.shape) == (nq, k)
                    assert torch.equal(i, wi), (N, M, nq, k, S, excl is not None)
                    assert torch.equal(v.view(torch.int32), wv.view(torch.int32)), (N, M, nq, k, S, excl is not None)
                    assert bool((i[torch.isneginf(v)] == -1).all())


# ---- Searcher and the command line, end to end -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w, before = W.make_world(tmp_path_factory.mktemp("search_admit_world"))
    yield w
    if before is None:
        os.environ.pop("SPRC_BERT_VOCAB", None)
    else:
        os.environ["SPRC_BERT_VOCAB"] = before


@pytest.fixture(scope="module")
def loaded(world):
    from sprc_amd.blip_validate import _load
    model, _ = _load("blip2_cir_align_prompt", "pretrain", str(world["root"] / "ckpt.pt"), "fp16", W.DEPTH)
    return model


class _Single:
    """The single-query answers, each computed once: search([ref], [cap], within=, exclude=, exclude_reference=)."""

    def __init__(self, s):
        self.s, self.memo = s, {}

    def __call__(self, ref, cap, k, within, exclude, exclude_reference):
        key = (str(ref), cap, k, None if within is None else tuple(within), None if exclude is None else tuple(exclude), exclude_reference)
        if key not in self.memo:
            self.memo[key] = self.s.search([ref], [cap], k=k, within=within, exclude=exclude, exclude_reference=exclude_reference)[0]
        return self.memo[key]


def _same(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print(f"[{what}] query {b}: got {g}\n    want {w}")
    assert len(got) == len(want) and got == want, what


def test_searcher_within_each_and_exclude_each(world, loaded):
    from sprc_amd.search import Searcher
    s = Searcher(loaded, world["store"])
    single = _Single(s)
    names = world["names"]
    # two queries, each its own list and its own exclusions; the reference leaves as well
    refs, caps = ["item-005", "item-011"], W.CAPTIONS[:2]
    within = [["item-009", "item-002", "item-005", "item-013", "item-007"], names[6:]]
    exclude = [["item-002"], ["item-013", "item-006"]]
    for xr in (False, True):
        got = s.search(refs, caps, k=10, within_each=within, exclude_each=exclude, exclude_reference=xr)
        _same(got, [single(r, c, 10, w, x, xr) for r, c, w, x in zip(refs, caps, within, exclude)], f"two queries, exclude_reference={xr}")
    assert [len(h) for h in got] == [3, 5]                                          # 5 - 1 - the reference; 8 - 2 - the reference
    # a None entry beside a list, on both sides; a shared `within` and `exclude` on top; a query that admits 3 images at k = 10
    got = s.search(refs, caps, k=10, within_each=[None, ["item-001", "item-002", "item-003"]], exclude_each=[["item-000"], None])
    _same(got, [single(refs[0], caps[0], 10, None, ["item-000"], False), single(refs[1], caps[1], 10, ["item-001", "item-002", "item-003"], None, False)],
          "None entries")
    assert [len(h) for h in got] == [10, 3]
    got = s.search(refs, caps, k=4, within=names[:9], exclude=["item-003"], within_each=[names[2:], None], exclude_reference=True)
    _same(got, [single(refs[0], caps[0], 4, names[2:9], ["item-003"], True), single(refs[1], caps[1], 4, names[:9], ["item-003"], True)],
          "shared and per-query filters")
    got = s.search(refs, caps, k=10, exclude_each=[None, None])                     # no restriction at all, through the admit path
    _same(got, [single(r, c, 10, None, None, False) for r, c in zip(refs, caps)], "all-admitting words")
    # a reference given as a file, and search_ids' own return value
    files = [world["files"]["item-005"], "item-011"]
    got = s.search(files, caps, k=10, within_each=within, exclude_reference=True)
    _same(got, [single(f, c, 10, w, None, True) for f, c, w in zip(files, caps, within)], "file reference")
    assert len(got[0]) == 5 and len(got[1]) == 7                                    # a file is no gallery name: nothing to leave out
    # 40 queries: two blocks of 32 with different unions (the first block's lists lie in the first 8 names, the second's in the last 8)
    refs40 = [names[(3 * b) % W.N_IMG] for b in range(40)]
    caps40 = [W.CAPTIONS[b % 4] for b in range(40)]
    within40 = [(names[:8] if b < 32 else names[6:])[b % 3:][:3 + b % 4] for b in range(40)]
    exclude40 = [None if b % 3 else [within40[b][1]] for b in range(40)]
    got = s.search(refs40, caps40, k=10, within_each=within40, exclude_each=exclude40, exclude_reference=True)
    _same(got, [single(r, c, 10, w, x, True) for r, c, w, x in zip(refs40, caps40, within40, exclude40)], "40 queries")
    assert {n for h in got[:32] for n, _ in h} <= set(names[:8]) and {n for h in got[32:] for n, _ in h} <= set(names[6:])
    # removed rows fold into the admit words
    before = single(refs[0], caps[0], 10, within[0], None, False)
    s.remove(["item-002"])
    got = s.search(refs, caps, k=10, within_each=[sorted(names.index(n) for n in within[0]), None])      # as rows: the removed one among them
    assert got[0] == [(n, v) for n, v in before if n != "item-002"] and len(got[0]) == 4
    assert len(got[1]) == 10 and "item-002" not in {n for n, _ in got[1]}
    # errors are raised on the host, before any device call (tests/test_search_admit_host.py runs them with no device at all)
    for kw, err in ((dict(within_each=[["item-001"], ["item-011"]], exclude_reference=True), ValueError),
                    (dict(within_each=[["item-001"]], exclude_each=None), ValueError), (dict(exclude_each=[None] * 3), ValueError),
                    (dict(within_each=[None, ["nope"]]), KeyError), (dict(within_each=[None, ["item-002"]]), KeyError)):
        with pytest.raises(err):
            s.search(refs, caps, k=3, **kw)
    with pytest.raises(ValueError, match="query 1:"):
        s.search(refs, caps, k=3, within_each=[["item-001"], ["item-011"]], exclude_reference=True)


def test_batch_command(world, loaded, capsys, tmp_path):
    from sprc_amd import search
    from sprc_amd.search import Searcher
    s = Searcher(loaded, world["store"])
    names = world["names"]
    lines = [
        {"reference": "item-005", "caption": W.CAPTIONS[0], "within": ["item-009", "item-002", "item-005", "item-013", "item-007"], "exclude_reference": True},
        {"reference_image": str(world["files"]["item-011"]), "caption": W.CAPTIONS[1], "within_glob": "item-00*", "exclude": ["item-003"]},
        {"reference": "item-001", "caption": W.CAPTIONS[2]},
        {"reference": "item-012", "caption": W.CAPTIONS[3], "within": names[4:], "within_glob": "item-01?", "exclude": ["item-010"], "exclude_reference": True},
        {"reference": "item-007", "caption": W.CAPTIONS[0], "exclude": ["item-000", "item-013"], "exclude_reference": False},
    ]
    qfile = tmp_path / "queries.jsonl"
    qfile.write_text(json.dumps(lines[0]) + "\n\n" + "\n".join(json.dumps(l) for l in lines[1:]) + "\n")
    line_no = [1, 3, 4, 5, 6]
    glob0 = [n for n in names if n.startswith("item-00")]
    want = [s.search(["item-005"], [W.CAPTIONS[0]], k=6, within=lines[0]["within"], exclude_reference=True)[0],
            s.search([world["files"]["item-011"]], [W.CAPTIONS[1]], k=6, within=glob0, exclude=["item-003"])[0],
            s.search(["item-001"], [W.CAPTIONS[2]], k=6)[0],
            s.search(["item-012"], [W.CAPTIONS[3]], k=6, within=["item-010", "item-011", "item-012", "item-013"], exclude=["item-010"], exclude_reference=True)[0],
            s.search(["item-007"], [W.CAPTIONS[0]], k=6, exclude=["item-000", "item-013"])[0]]
    assert [len(h) for h in want] == [4, 6, 6, 2, 6]
    cmd = ["batch", "--index", world["store"], "--queries", str(qfile), "-k", "6"] + world["base"]
    capsys.readouterr()
    got = search.main(cmd)
    printed = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines() if l.startswith("{\"line\"")]
    _same(got, want, "batch 32")
    assert [p["line"] for p in printed] == line_no and [p["caption"] for p in printed] == [l["caption"] for l in lines]
    assert [p["reference"] for p in printed] == [l.get("reference") or l["reference_image"] for l in lines]
    assert [[(r["rank"], r["name"], r["score"]) for r in p["results"]] for p in printed] == [[(i + 1, n, v) for i, (n, v) in enumerate(h)] for h in want]
    out = tmp_path / "answers.jsonl"
    got2 = search.main(cmd + ["--batch", "2", "--out", str(out)])
    _same(got2, got, "batch 2")
    assert [json.loads(l) for l in out.read_text().splitlines()] == printed
    assert "\"line\"" not in capsys.readouterr().out                                # --out: nothing on stdout
    # no filters at all: the unfiltered path's results
    plain = tmp_path / "plain.jsonl"
    plain.write_text("".join(json.dumps({k: l[k] for k in ("reference", "reference_image", "caption") if k in l}) + "\n" for l in lines))
    refs = [l.get("reference") or world["files"]["item-011"] for l in lines]
    got = search.main(["batch", "--index", world["store"], "--queries", str(plain), "-k", "6", "--out", str(out)] + world["base"])
    _same(got, s.search(refs, [l["caption"] for l in lines], k=6), "no filters")
    # an empty set names its line, an unknown name too
    bad = tmp_path / "bad.jsonl"
    bad.write_text(json.dumps(lines[2]) + "\n" + json.dumps({"reference": "item-001", "caption": "a", "within": ["item-001"], "exclude_reference": True}) + "\n")
    with pytest.raises(ValueError, match="line 2:"):
        search.main(["batch", "--index", world["store"], "--queries", str(bad)] + world["base"])
