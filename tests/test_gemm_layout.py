"""Host check of the GEMM layout tier (tests/_gemm_layout.py), so that tests/test_gemm_layout_gpu.py cannot pass because its own
construction went wrong: the case table reaches every epilogue store path of every tile kernel through every condition that selects
it; the checker passes on an emulated correct kernel and fails on each planted addressing fault; the restated dispatcher gives the
hand-derived routes; and the argument checks that guard the kernels' 32-bit tile offsets reject what they must without launching."""
import ctypes as C

import pytest
import torch

import _gemm_layout as G
from sprc_amd import _lib as L

TABLE = {t: G.forced_cases(t) for t in G.TILES}
ALL = [c for t in G.TILES for c in TABLE[t]]
CLASSES = {4: {"w4", "scalar"}, 2: {"w8", "w4", "scalar"}, 1: {"w8", "w4", "scalar"}}


def test_every_case_is_a_legal_layout():
    names = set()
    for c in ALL + G.auto_cases():
        assert c.name not in names
        names.add(c.name)
        es = G.ES_OP[c.op]
        assert c.a_pad % 16 == 0 and c.w_pad % 16 == 0 and (c.krow * es) % 16 == 0            # the ABI: 16-byte rows and bases
        if c.kind == "sim":
            assert c.ldc > c.N // 32
            continue
        assert c.a_pad > 0 and c.w_pad > 0 and c.ldc > (2 * c.N if c.out == "x3" else c.N)
        assert c.c_off in (0, 1, 2, 4) and c.bias_off in (0, 1) and c.r_off in (0, 1, 4)
        if c.resid == "own":
            assert c.ldr > c.N and c.ldr != c.ldc
        for mp in (c.amap, c.cmap):
            if mp is not None:
                rpg, stride, offs = mp
                assert rpg in (1, 32, 64) and stride > rpg and all(o > 0 for o in offs) and (rpg == 1 or c.M % rpg != 0)
        if c.kind == "pair":                            # the two products write disjoint rows
            r0, r1 = (set(G.phys_rows(c.cmap, p, c.M).tolist()) for p in (0, 1))
            assert not (r0 & r1) and c.amap[2][0] != c.amap[2][1]
    assert any(p % 16 == 0 and p & (p - 1) for c in ALL for p in (c.a_pad, c.w_pad))             # pads that are no power of two
    assert {c.M for c in ALL if c.kind != "sim" and not c.name.startswith("t1-big")} == set(G.M_SET)
    assert {4, 8, 12, 36, 130, 264, 516} <= {c.N for c in ALL}


def test_every_forced_case_reaches_the_kernel_it_names_at_256_and_at_64_cus():
    """No case may be skipped on a 256-CU MI355X (nor on a 64-CU partition of one): the route does not depend on the CU count there."""
    for c in ALL:
        for ncu in (256, 64):
            assert G.expected_route(c.M, c.N, c.K, ncu, **c.route_args()) == c.kernel, (c.name, ncu)
    per_tile = {t: {c.kernel for c in TABLE[t]} for t in G.TILES}
    assert per_tile == {1: {"k64r", "k64s", "k128"}, 2: {"k128"}, 4: {"anti", "lock256"}, 14: {"lock256", "k128"}}
    # the fall-throughs: max32 and fp8 under 1, split rows under 14
    assert {c.kernel for c in TABLE[1] if c.kind == "sim" or c.op in ("fp8", "f32")} == {"k128"}
    assert {c.kernel for c in TABLE[14] if c.op == "mix"} == {"k128"} and {c.kernel for c in TABLE[4] if c.op == "f32"} == {"lock256"}


def test_hand_derived_routes_of_the_automatic_cases():
    """At 64 CUs, N = 4096 (16 256-tiles, 32 128-tiles per panel), M = 1124: 128x128 costs 288 tiles = 2 full rounds + 32 -> 1.82;
    256x256 costs ceil(80 / 64) = 2; peeling 1024 rows costs 1 + 0.42 (32 tiles of the 100 remainder rows) + 0.08 = 1.5 < 1.82 - 0.25.
    The remainder: split-K with scratch at K >= 4096, else the 64x64 ring (32 <= 64 tiles); fp8 operands have no 64x64 tile: 128x128.
    A short reduction with an fp32 + residual epilogue weighs 256x256 rounds by 1.35: 1.35 + 0.42 + 0.08 + 0.25 > 1.82, no peel."""
    kw = dict(op="bf16", out="f32", resid=True, ldc=4104)
    assert G.expected_route(1124, 4096, 4096, 64, scratch_floats=8 * 100 * 4096, **kw) == "peel:anti+splitk"
    assert G.expected_route(1124, 4096, 4096, 64, scratch_floats=8 * 100 * 4096 - 1, **kw) == "peel:anti+k64r"
    assert G.expected_route(1124, 4096, 4096, 64, **kw) == "peel:anti+k64r"
    assert G.expected_route(1124, 4096, 256, 64, op="fp8", out="bf16", resid=True) == "peel:anti+k128"
    assert G.expected_route(1124, 4096, 256, 64, op="fp8", out="f32", resid=True) == "k128"
    assert G.expected_route(1324, 4096, 2048, 64, op="bf16", out="bf16") == "anti"                # 96 remainder tiles: 1.78 + 0.25 > 2
    assert G.peel_rows(1124, 4096, 4096, 64, op="bf16") == 1024
    assert G.expected_route(1124, 4096, 4096, 64, mapped=True, **kw) != "peel:anti+k64r"          # row maps never peel
    assert G.expected_route(1124, 4096, 4096, 256, **kw) == "k128"                               # the whole chip: 288 tiles, one round
    # the existing split-K test's shape on the whole chip (tests/test_ops_gpu.py::test_gemm_bf16_splitk_remainder)
    assert G.expected_route(4196, 4096, 4096, 256, op="bf16", scratch_floats=8 * 128 * 4096) == "peel:anti+splitk"
    assert G.expected_route(300, 384, 128, 256, op="fp8") == "k128" and G.expected_route(70, 96, 32, 256, op="f32") == "k128"
    for c in G.auto_cases():
        sf = 8 * (c.M - G.peel_rows(c.M, c.N, c.K, G.AUTO_NCU, op=c.op, out=c.out, resid=c.resid is not None)) * c.N if c.scratch else 0
        assert G.expected_route(c.M, c.N, c.K, G.AUTO_NCU, scratch_floats=sf, **c.route_args()) == c.kernel, c.name
        assert G.epi_class(c) == G.epi_class(G.contiguous_case(c)), c.name                         # main rows: bit for bit
    assert {c.kernel for c in G.auto_cases()} == {"peel:anti+splitk", "peel:anti+k64r", "peel:anti+k128"}


def test_the_table_reaches_every_store_path_of_every_kernel_through_every_cause():
    seen, causes, feats = {}, {}, {}
    for c in ALL:
        if c.kind == "sim":
            continue
        cls = G.epi_class(c)
        seen.setdefault((c.kernel, c.out), set()).add(cls)
        for cause in G.class_causes(c):
            if len(G.class_causes(c)) == 1:              # the cause acts alone
                causes.setdefault((cls, G.ES_OUT[c.out] < 4 or c.out == "x3"), set()).add(cause)
        f = feats.setdefault(c.kernel, set())
        f |= {"amap"} if c.amap else set()
        f |= {"cmap"} if c.cmap else set()
        f |= {"pair"} if c.kind == "pair" else set()
        f |= {"ldr"} if c.resid == "own" and c.ldr != c.ldc else set()
        f |= {"alias"} if c.resid == "alias" else set()
        f |= {"nobias"} if not c.bias else set()
        f |= {"noresid"} if c.resid is None else set()
    outs_of = {"k64r": {"f32", "bf16", "f16", "x3"}, "k64s": {"f32", "bf16", "f16", "x3"}, "k128": {"f32", "bf16", "f16", "fp8", "x3"},
               "anti": {"f32", "bf16", "f16", "fp8", "x3"}, "lock256": {"f32", "bf16", "f16", "fp8", "x3"}}
    for kern in G.KERNELS:
        for out in outs_of[kern]:
            assert seen.get((kern, out)) == CLASSES[G.ES_OUT[out]], (kern, out, seen.get((kern, out)))
        assert {"amap", "cmap", "ldr", "alias", "nobias", "noresid"} <= feats[kern], (kern, feats[kern])
    assert all("pair" in feats[k] for k in ("k64r", "k128", "anti", "lock256"))
    assert causes[("scalar", False)] == {"n", "ldc", "ldr", "calign", "bias", "ralign"}             # fp32 output
    assert causes[("scalar", True)] == {"n", "ldc", "ldr", "calign", "bias", "ralign"}              # outputs narrower than fp32
    assert causes[("w4", True)] == {"n", "ldc", "calign"}
    # every operand / output / activation combination dispatch and dispatch_mix build runs on every tile value it is built for
    for t in G.TILES:
        got = {(c.op, c.out, c.act) for c in TABLE[t] if c.kind != "sim"}
        assert got == {(op, out, a) for op, out, acts, _, _ in G.COMBOS for a in acts}, t
        assert {c.op for c in TABLE[t] if c.kind == "sim"} == {"bf16", "f16", "f32"}


# ---- the checker on an emulated kernel ----------------------------------------------------------------------------------------------------
def _pick(pred):
    return next(c for c in ALL if pred(c))


SELF_TEST = {
    "both maps, own residual": lambda c: c.amap and c.cmap and c.resid == "own" and c.ldc < c.ldr and c.out == "f32" and c.M > 64 and c.kind == "gemm",
    "paired": lambda c: c.kind == "pair" and c.out == "bf16" and c.M > 64,
    "aliased": lambda c: c.resid == "alias" and c.cmap and c.M > 64,
    "split rows": lambda c: c.out == "x3" and c.op == "mix" and c.cmap and c.M > 64,
    "fp8": lambda c: c.out == "fp8" and c.resid == "own" and c.M > 64,
    "max32": lambda c: c.kind == "sim" and c.op == "bf16",
}


@pytest.mark.parametrize("which", list(SELF_TEST))
def test_the_checker_passes_on_an_emulated_kernel(which):
    c = _pick(SELF_TEST[which])
    d = G.build(c)
    Cb, Rb = G.emulate(c, d)
    assert G.check(c, d, Cb, Rb) == [], c.name
    assert bool((Cb != d.C.buf).any())
    # the contiguous twin holds the same logical problem: the same stored bytes
    for p in range(c.nprod):
        t = G.contiguous_case(c, p)
        dt = G.build(t)
        dt.out_scale = d.out_scale
        Ct, Rt = G.emulate(t, dt)
        assert G.check(t, dt, Ct, Rt) == []
        assert torch.equal(G.written_rows(t, dt, Ct)[0], G.written_rows(c, d, Cb)[p]), (c.name, p)


FAULTS = [("pad_col", "both maps, own residual", "guard"), ("guard_row", "both maps, own residual", "guard"),
          ("between_rows", "both maps, own residual", "guard"), ("row_unmapped", "both maps, own residual", "guard"),
          ("row_unmapped", "both maps, own residual", "poison"), ("resid_ldc", "both maps, own residual", ""),
          ("a_pad", "both maps, own residual", "poison"), ("a_pad", "split rows", "poison"), ("lo_at_hi8", "split rows", "poison"),
          ("pad_col", "split rows", "guard"), ("pad_col", "max32", "guard"), ("between_rows", "paired", "guard")]


@pytest.mark.parametrize("fault,which,kind", FAULTS, ids=[f"{f[0]}-{f[1].split()[0]}-{f[2] or 'any'}" for f in FAULTS])
def test_the_checker_fails_on_each_planted_fault(fault, which, kind):
    c = _pick(SELF_TEST[which])
    d = G.build(c)
    bad = G.check(c, d, *G.emulate(c, d, fault=fault))
    assert bad and any(m.split(": ")[-2 if m.startswith("product") else 0].startswith(kind) or kind in m for m in bad), (c.name, bad)


def test_a_wrong_value_of_order_one_breaks_every_bound():
    """Bias is distinct per column and the residual per element: a misplaced row or column is an error of order 1 -- far outside every
    bound the cases take (the widest is bf16 output: 4e-2 + 1.6e-2 |x|)."""
    for which in ("both maps, own residual", "paired", "split rows", "aliased"):
        c = _pick(SELF_TEST[which])
        d = G.build(c)
        ref = G.reference(c, d)[0]
        rolled = G.encode_out(torch.roll(ref, 1, dims=1), c.out)                       # every column one to the right
        assert G.check_values(c, rolled, ref), c.name
        if c.M > 1:
            assert G.check_values(c, G.encode_out(torch.roll(ref, 1, dims=0), c.out), ref), c.name


# ---- argument checks that launch nothing ------------------------------------------------------------------------------------------------
def _args(**kw):
    g = L.GemmArgs()
    g.M, g.N, g.K, g.dtype, g.out_dtype = 1, 8, 64, L.SPRC_BF16, L.SPRC_F32
    g.A, g.W, g.C, g.lda, g.ldw, g.ldc = 0x10000, 0x20000, 0x30000, 64, 64, 8       # never dereferenced: every call below returns before a launch
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _rc(g, b=None):
    lib = L.load()
    rc = lib.sprc_gemm(C.byref(g), None) if b is None else lib.sprc_gemm_pair(C.byref(g), C.byref(b), None)
    return rc, lib.sprc_last_error().decode()


def test_w_scale_must_be_16_byte_aligned():
    rc, msg = _rc(_args(dtype=L.SPRC_FP8, K=128, lda=128, ldw=128, w_scale=0x40004, a_scale=1.0))
    assert rc == -1 and "w_scale" in msg and "aligned" in msg


@pytest.mark.parametrize("field", ["amap", "cmap"])
@pytest.mark.parametrize("stride,offset", [(-64, 0), (64, -1), (-64, -64)])
def test_negative_row_map_fields_are_rejected(field, stride, offset):
    rc, msg = _rc(_args(**{field: L.RowMap(32, stride, offset)}))
    assert rc == -4 and "row-map" in msg, msg
    a, b = _args(**{field: L.RowMap(32, 64, 0)}), _args(**{field: L.RowMap(32, 64, -3)})
    if stride > 0:                                  # the second product's offset of a paired launch
        rc, msg = _rc(a, b)
        assert rc == -4 and "row-map" in msg, msg


def test_epilogue_range_rejections():
    rc, msg = _rc(_args(ldc=1 << 24))
    assert rc == -4 and "ldc" in msg
    rc, msg = _rc(_args(resid=0x50000, ldr=1 << 24))
    assert rc == -4 and "ldr" in msg
    rc, msg = _rc(_args(cmap=L.RowMap(32, 31, 0)))              # a cmap stride below its rows per group: not monotone
    assert rc == -4 and "stride" in msg
    rc, msg = _rc(_args(cmap=L.RowMap(32, 1 << 23, 0)))
    assert rc == -4
