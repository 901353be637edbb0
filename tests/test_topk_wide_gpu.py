"""sprc_topk_wide on the GPU: top-k for 1 <= k <= 256 with an optional left-out column, bit for bit against the ranking contract
restated in numpy on the same fp32 rows -- 64-bit keys (order-preserving image of fl32(1 - sim), id), ascending -- and against
oracle.sprc_oracle.topk_stable where no id array is involved.  Shapes: every k / N on both sides of the wave (64), of the step
(256), of k itself (padding when k > N), several steps, and 300 rows in one launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sprc_oracle as O  # noqa: E402
from sprc_amd import engine as E  # noqa: E402
from sprc_amd._lib import SprcError  # noqa: E402

DEV = "cuda:0"
KS = (1, 64, 65, 128, 200, 256)
NS = (1, 63, 64, 65, 199, 200, 201, 256, 257, 513, 5000)
NQ = 5


def dist_bits(sim: np.ndarray) -> np.ndarray:
    """The order-preserving integer image of fl32(1 - sim): NaN last, -0.0 as +0.0."""
    with np.errstate(invalid="ignore"):
        d = (np.float32(1.0) - sim.astype(np.float32)).astype(np.float32) + np.float32(0.0)
    u = d.view(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(d), np.uint32(0xFFFFFFFF), bits).astype(np.uint64)


def expected(sim: np.ndarray, k: int, gidx=None, idx_base: int = 0, skip=None):
    """-> (vals[nq,k] fp32, idx[nq,k] int32): the k smallest keys of every row, the skipped column deleted."""
    nq, N = sim.shape
    ids = gidx.astype(np.int64) if gidx is not None else np.arange(N, dtype=np.int64)[None, :].repeat(nq, 0) + idx_base
    key = (dist_bits(sim) << np.uint64(32)) | (ids.astype(np.uint32).astype(np.uint64))
    vals = np.full((nq, k), -np.inf, dtype=np.float32)
    idx = np.full((nq, k), -1, dtype=np.int32)
    for q in range(nq):
        cols = np.arange(N)
        if skip is not None and 0 <= skip[q] < N:
            cols = np.delete(cols, skip[q])
        o = cols[np.argsort(key[q, cols], kind="stable")][:k]
        vals[q, :len(o)], idx[q, :len(o)] = sim[q, o], ids[q, o]
    return vals, idx


def check(sim: np.ndarray, k: int, gidx=None, idx_base: int = 0, skip=None, ld=None):
    nq, N = sim.shape
    if ld is None:
        t = torch.from_numpy(sim).to(DEV)
    else:                                   # rows of a wider matrix whose other columns hold values that would win
        wide = torch.full((nq, ld), 9.0, dtype=torch.float32, device=DEV)
        wide[:, :N] = torch.from_numpy(sim).to(DEV)
        t = wide[:, :N]
    g = None if gidx is None else torch.from_numpy(gidx).to(DEV)
    s = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.int32)).to(DEV)
    vals, idx = E.topk_wide(t, k, gidx=g, idx_base=idx_base, skip=s)
    want_v, want_i = expected(sim, k, gidx, idx_base, skip)
    what = f"k={k} N={N} ld={ld} gidx={gidx is not None} base={idx_base} skip={None if skip is None else list(skip)}"
    assert np.array_equal(idx.cpu().numpy(), want_i), what
    assert np.array_equal(vals.cpu().numpy().view(np.int32), want_v.view(np.int32)), what      # bits: NaN compares too
    return vals, idx


def rows(kind: str, N: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    sim = rng.uniform(-0.2, 0.9, size=(NQ, N)).astype(np.float32)
    if kind == "grid":                      # many exact ties, across the k-th place too
        sim = (np.round(sim * 16) / 16).astype(np.float32)
    elif kind == "ascending":               # every step beats what came before: every step passes
        sim = np.sort(sim, axis=1)
    elif kind == "descending":              # the best come first: after k elements no step passes
        sim = np.sort(sim, axis=1)[:, ::-1].copy()
    elif kind == "special":
        vals = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1.0, 2.0], dtype=np.float32)
        hit = rng.uniform(size=sim.shape) < 0.3
        sim = np.where(hit, vals[rng.integers(0, len(vals), size=sim.shape)], sim).astype(np.float32)
    return sim


@pytest.mark.parametrize("N", NS)
def test_random_rows_every_k_with_ld_gidx_and_base(N):
    sim = rows("random", N, seed=N)
    gidx = np.random.default_rng(N + 1).permutation(10 * N + 7)[:NQ * N].reshape(NQ, N).astype(np.int32)
    for k in KS:
        check(sim, k)
        check(sim, k, ld=N + 3)
        check(sim, k, gidx=gidx)
        check(sim, k, idx_base=1000003)
        _, want = O.topk_stable(sim, k)
        got = E.topk_wide(torch.from_numpy(sim).to(DEV), k)[1].cpu().numpy()
        assert np.array_equal(got[:, :min(k, N)], want) and (got[:, min(k, N):] == -1).all()


@pytest.mark.parametrize("kind", ["grid", "ascending", "descending", "special"])
def test_ties_sorted_rows_and_special_values(kind):
    for N in NS:
        sim = rows(kind, N, seed=100 + N)
        gidx = np.stack([np.random.default_rng(7 * N + q).permutation(N) for q in range(NQ)]).astype(np.int32)
        for k in KS:
            check(sim, k)
            check(sim, k, gidx=gidx, ld=N + 1)


@pytest.mark.parametrize("kind", ["random", "grid"])
def test_skip_deletes_one_column(kind):
    for N in NS:
        sim = rows(kind, N, seed=200 + N)
        order = O.rank_stable(sim)
        for k in KS:
            skip = [0, N - 1, int(order[2, 0]), int(order[3, min(k, N) - 1]), -1]
            check(sim, k, skip=skip)
            check(sim, k, skip=skip, idx_base=17, ld=N + 2)
    sim = rows("random", 300, seed=5)
    assert torch.equal(E.topk_wide(torch.from_numpy(sim).to(DEV), 200, skip=torch.full((NQ,), -5))[1],
                       E.topk_wide(torch.from_numpy(sim).to(DEV), 200)[1])


@pytest.mark.parametrize("kind", ["random", "grid", "special"])
def test_same_bits_as_topk_up_to_64(kind):
    for N in NS:
        sim = torch.from_numpy(rows(kind, N, seed=300 + N)).to(DEV)
        gidx = torch.from_numpy(np.stack([np.random.default_rng(N + q).permutation(N) for q in range(NQ)]).astype(np.int32)).to(DEV)
        for k in (1, 7, 51, 64):
            for kw in ({}, {"idx_base": 5}, {"gidx": gidx}):
                v0, i0 = E.topk(sim, k, **kw)
                v1, i1 = E.topk_wide(sim, k, **kw)
                assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32)), (kind, N, k, list(kw))


def test_bad_arguments_are_errors():
    sim = torch.zeros((2, 10), dtype=torch.float32, device=DEV)
    for k in (0, 257):
        with pytest.raises(SprcError, match="sprc_topk_wide"):
            E.topk_wide(sim, k)
    from sprc_amd import _lib as L
    out_v, out_i = torch.empty((2, 4), device=DEV), torch.empty((2, 4), dtype=torch.int32, device=DEV)
    lib = L.load()
    assert lib.sprc_topk_wide(sim.data_ptr(), 9, None, 0, None, 2, 10, 4, out_v.data_ptr(), out_i.data_ptr(), None) != 0     # ld < N
    assert lib.sprc_topk_wide(sim.data_ptr(), 10, None, 0, None, 2, 0, 4, out_v.data_ptr(), out_i.data_ptr(), None) != 0    # N < 1


def test_300_rows_in_one_launch():
    rng = np.random.default_rng(9)
    sim = rng.uniform(-0.2, 0.9, size=(300, 5000)).astype(np.float32)
    sim[::3] = (np.round(sim[::3] * 16) / 16).astype(np.float32)
    skip = rng.integers(-1, 5000, size=300).astype(np.int32)
    t = torch.from_numpy(sim).to(DEV)
    for k in (200, 256):
        vals, idx = E.topk_wide(t, k, skip=torch.from_numpy(skip))
        want_v, want_i = expected(sim, k, skip=skip)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(vals.cpu().numpy(), want_v)
