"""Every `extern "C"` entry point of csrc/train.hip (and the two loss forwards of csrc/rowops.hip it differentiates) ALONE, at the shape,
stride and accumulate edges the model never visits: tile and loop remainders, leading dimensions different from the logical width
(sentinel-guarded: tests/_train_ref.py `Guard`), `+=` outputs that start from non-zero values, arg-max ties, colliding scatter rows,
attention-probability dropout regenerated in the backward, and `train._Linear.bwd` in both product modes.  References: the same
operation in torch on the CPU in float64 (autograd for the gradients), never another kernel of this library.

Bars.  Bit-exact: the transposes, jstar, dropout masks, the pre-LN embedding rows (one fp32 add), sentinels, refusals.  Derived
(`_train_ref.sum_bound`: 2 n 2^-24 sum|term| + 1 ulp): colsum, the embedding scatters, dfusion / dfeats, align_mse_bwd, and dW / db / dx
of the linear.  Calibrated (`_train_ref.calibrated`: kernel error <= 4 x torch's fp32 CPU error, both against fp64): the rest.

Largest e_kernel / e_torch per kernel output, measured on the MI355X with the kernels as they were before this file existed
(the last test prints the table of the session):
    gelu_fwd: y                        0.19
    gelu_bwd: dx                       0.68
    layernorm_bwd: dx                  1.55
    layernorm_bwd: dgamma              1.62
    layernorm_bwd: dbeta               2.21
    attention (fp32 forward): out      2.46
    attention_bwd: dq                  2.43
    attention_bwd: dk                  2.71
    attention_bwd: dv                  2.61
    contrastive_ce: loss               1.53 (0.69 after the batch-of-one fix)
    contrastive_ce_bwd: dsim           1.25
    contrastive_ce_bwd: dtemp          2.17
    l2norm_bwd: dx                     1.51
    l2norm_bwd: dx, all-zero row       0.82
    align_mse: loss                    1.35
None exceeds the bar; the l2norm figure is with the floor at the subtracted terms (see test_l2norm_bwd), DESIGN.md section 4.4 has the notes.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import _train_ref as R
from sprc_amd import _lib as L

gpu = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F = torch.nn.functional
GRID_CAP = 4096 * 256                    # elements one pass of a capped 1-D grid covers (grid1d: 4096 blocks of 256 threads)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(*seed):
    return torch.Generator().manual_seed(hash(tuple(seed)) % (1 << 31))


def _rn(g, *shape):
    return torch.randn(shape, generator=g)


def _g(rows, cols, ld, data=None, fill=R.SENTINEL, dtype=torch.float32):
    return R.strided(rows, cols, ld, fill, dtype, DEV, data)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _ok(rc, what=""):
    L.check(rc, what)


def _refused(rc, word=None):
    assert rc == -1, rc
    if word is not None:
        assert word in L.load().sprc_last_error(), L.load().sprc_last_error()


# ---- 1. transposes --------------------------------------------------------------------------------------------------------------
_f32 = lambda v: float(np.float32(v))                                              # noqa: E731
SPECIALS = [0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -14 - 2.0 ** -24,   # fp16 subnormals and their ties
            65504.0, 65520.0, -65520.0, _f32(np.nextafter(np.float32(65520), np.float32(0))), 1e5,        # 65520 is the tie that rounds to fp16 inf
            1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11),                                        # fp16 round-to-even ties
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8), 3.4e38,                               # bf16 ties; rounds to bf16 inf
            float("inf"), float("-inf")]


@gpu
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 70])
def test_transposes_are_bit_exact_with_padded_leading_dimensions(rows):
    lib = L.load()
    for cols in (1, 32, 33, 133):
        x = _rn(_gen(1, rows, cols), rows, cols)
        flat = x.view(-1)
        sp = torch.tensor(SPECIALS)
        flat[(torch.arange(len(sp)) * 5) % flat.numel()] = sp
        gs, src = _g(rows, cols, cols + 3, data=x)
        gs.seal()
        for dtype, tdt in ((None, torch.float32), (L.SPRC_F16, torch.float16), (L.SPRC_BF16, torch.bfloat16)):
            gd, dst = _g(cols, rows, rows + 5, fill=NAN, dtype=tdt)
            gd.seal()
            if dtype is None:
                _ok(lib.sprc_transpose_f32(src.data_ptr(), cols + 3, dst.data_ptr(), rows + 5, rows, cols, _st()), "sprc_transpose_f32")
            else:
                _ok(lib.sprc_transpose_f32_to16(src.data_ptr(), cols + 3, dst.data_ptr(), rows + 5, rows, cols, dtype, _st()), "sprc_transpose_f32_to16")
            torch.cuda.synchronize()
            assert torch.equal(_bits(dst), _bits(x.t().to(tdt))), (rows, cols, tdt)
            assert gd.outside_intact() and gs.outside_intact(whole=True), (rows, cols, tdt)      # columns rows .. ld_dst of every row included


# ---- 2. column sums ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [1, 7, 8, 9, 25, 32, 33, 57, 200])
def test_colsum_overwrites_or_accumulates(M):
    lib = L.load()
    for N in (1, 31, 32, 33, 100):
        x = _rn(_gen(2, M, N), M, N)
        gx, xd = _g(M, N, N + 5, data=x)
        gx.seal()
        ref, tabs = x.double().sum(0), x.double().abs().sum(0)
        # accumulate = 0 over NaN: must overwrite
        go, out = _g(1, N, N, fill=NAN)
        go.seal()
        _ok(lib.sprc_colsum_f32(xd.data_ptr(), N + 5, M, N, out.data_ptr(), 0, _st()), "sprc_colsum_f32")
        R.assert_sum_bound(f"colsum M={M} N={N} overwrite", out[0], ref, M, tabs)
        assert go.outside_intact()
        # accumulate = 1 from non-zero values
        init = _rn(_gen(3, M, N), N) * 3
        go, out = _g(1, N, N, data=init)
        go.seal()
        _ok(lib.sprc_colsum_f32(xd.data_ptr(), N + 5, M, N, out.data_ptr(), 1, _st()), "sprc_colsum_f32")
        R.assert_sum_bound(f"colsum M={M} N={N} accumulate", out[0], init.double() + ref, M + 1, init.double().abs() + tabs)
        assert go.outside_intact() and gx.outside_intact(whole=True)


# ---- 3. GELU ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID_CAP + 3])
def test_gelu_forward_and_backward(n):
    lib = L.load()
    g = _gen(4, n)
    x, dy = _rn(g, n) * 3, _rn(g, n)
    fixed = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 5.0, -5.0, 10.0, -10.0, 40.0, -40.0])
    x[-min(n, len(fixed)):] = fixed[:min(n, len(fixed))]                        # at the END: n > the grid cap puts them on the grid-stride pass
    y64, (dx64,) = R.grads_of(R.gelu, [x], dy, torch.float64)
    y32, (dx32,) = R.grads_of(R.gelu, [x], dy, torch.float32)
    gx, xd = _g(1, n, n, data=x)
    gdy, dyd = _g(1, n, n, data=dy)
    gy, yd = _g(1, n, n, fill=NAN)
    gdx, dxd = _g(1, n, n, fill=NAN)
    for t in (gx, gdy, gy, gdx):
        t.seal()
    _ok(lib.sprc_gelu_fwd(xd.data_ptr(), yd.data_ptr(), n, _st()), "sprc_gelu_fwd")
    _ok(lib.sprc_gelu_bwd(xd.data_ptr(), dyd.data_ptr(), dxd.data_ptr(), n, _st()), "sprc_gelu_bwd")
    R.calibrated(f"gelu_fwd n={n}", yd, y64, y32, "gelu_fwd: y")
    R.calibrated(f"gelu_bwd n={n}", dxd, dx64, dx32, "gelu_bwd: dx")
    assert gy.outside_intact() and gdx.outside_intact() and gx.outside_intact(whole=True) and gdy.outside_intact(whole=True)


# ---- 4. LayerNorm backward ----------------------------------------------------------------------------------------------------------
def _ln_ws(M, D):
    """exactly sprc_layernorm_bwd_workspace_bytes(M, D) bytes, 16-byte aligned, inside a guarded byte buffer (0xFF: NaN as floats)"""
    need = int(L.load().sprc_layernorm_bwd_workspace_bytes(M, D))
    assert need == (M + 31) // 32 * 2 * D * 4
    g = R.Guard(32 + need + 32, 0xFF, torch.uint8, DEV)
    ws = g.view(32, (need,), (1,))
    assert ws.data_ptr() % 16 == 0
    return g.seal(), ws, need


@gpu
@pytest.mark.parametrize("D", [4, 252, 256, 260, 768, 1408, 2048])
def test_layernorm_bwd(D):
    lib = L.load()
    ldx, lddy, lddx = D + 4, D + 8, D + 12
    for M, eps in itertools.product((1, 8, 9, 31, 32, 33, 65), (1e-12, 1e-5)):
        g = _gen(5, M, D, int(eps * 1e13))
        x, gam, bet, dy = _rn(g, M, D) * 2 + 0.3, _rn(g, D) * 0.1 + 1, _rn(g, D) * 0.1, _rn(g, M, D)
        if eps == 1e-5:
            x[M // 2] = 0.5                                                    # a constant row: variance 0, rstd = eps^-1/2
        dg0, db0 = _rn(g, D), _rn(g, D)
        _, (dx64, dg64, db64) = R.grads_of(R.layer_norm(eps), [x, gam, bet], dy, torch.float64)
        _, (dx32, dg32, db32) = R.grads_of(R.layer_norm(eps), [x, gam, bet], dy, torch.float32)
        gx, xd = _g(M, D, ldx, data=x)
        gdy, dyd = _g(M, D, lddy, data=dy)
        gg, gd = _g(1, D, D, data=gam)
        for need_dx in ((True, False) if M in (9, 65) else (True,)):
            gdx, dxd = _g(M, D, lddx, fill=NAN)
            gdg, dgd = _g(1, D, D, data=dg0)
            gdb, dbd = _g(1, D, D, data=db0)
            gws, ws, need = _ln_ws(M, D)
            for t in (gx, gdy, gg, gdx, gdg, gdb):
                t.seal()
            _ok(lib.sprc_layernorm_bwd(xd.data_ptr(), ldx, gd.data_ptr(), dyd.data_ptr(), lddy, eps, M, D, dxd.data_ptr() if need_dx else None, lddx,
                                       dgd.data_ptr(), dbd.data_ptr(), ws.data_ptr(), need, _st()), "sprc_layernorm_bwd")
            tag = f"ln_bwd M={M} D={D} eps={eps:g} dx={int(need_dx)}"
            if need_dx:
                R.calibrated(tag + " dx", dxd, dx64, dx32, "layernorm_bwd: dx")
            else:
                assert gdx.outside_intact(whole=True)                           # dx = NULL: nothing written, the accumulators still right
            R.calibrated(tag + " dgamma", dgd, dg0.double() + dg64, dg0 + dg32, "layernorm_bwd: dgamma")
            R.calibrated(tag + " dbeta", dbd, db0.double() + db64, db0 + db32, "layernorm_bwd: dbeta")
            assert all(t.outside_intact() for t in (gdx, gdg, gdb, gws)) and all(t.outside_intact(whole=True) for t in (gx, gdy, gg)), tag


# ---- 5. attention forward (fp32) + backward -----------------------------------------------------------------------------------------
def _attn_case(B, H, Tq, Tk, mask, drop, qk_scale=0.5, tag=""):
    """q / k / v: column slices of one packed [rows, 3 H 64] sentinel buffer; dq / dk / dv: the same slices of a second (NaN) one; dout
    and the forward output with leading dimensions of their own; scratch of exactly the documented size."""
    lib = L.load()
    HD, scale = H * 64, 0.125
    g = _gen(6, B, H, Tq, Tk, drop is not None)
    q, k, v, do = _rn(g, B * Tq, HD) * qk_scale, _rn(g, B * Tk, HD) * qk_scale, _rn(g, B * Tk, HD), _rn(g, B * Tq, HD)
    keep, dscale = None, 1.0
    if drop is not None:
        p, seed, site = drop
        keep, dscale = R.keep_mask(seed, site, (B, H, Tq, Tk), p), R.drop_scale(p)
    fn = R.attention(B, H, Tq, Tk, scale, mask, keep, dscale)
    o64, g64 = R.grads_of(fn, [q, k, v], do, torch.float64)
    o32, g32 = R.grads_of(fn, [q, k, v], do, torch.float32)
    rows, ld = B * max(Tq, Tk), 3 * HD + 8
    gin, gout = R.Guard(R.LEAD + rows * ld + R.LEAD, R.SENTINEL, torch.float32, DEV), R.Guard(R.LEAD + rows * ld + R.LEAD, NAN, torch.float32, DEV)
    qd, kd, vd = (gin.view(R.LEAD + i * HD, (B * T, HD), (ld, 1)) for i, T in enumerate((Tq, Tk, Tk)))
    dq, dk, dv = (gout.view(R.LEAD + i * HD, (B * T, HD), (ld, 1)) for i, T in enumerate((Tq, Tk, Tk)))
    qd.copy_(q), kd.copy_(k), vd.copy_(v)
    gdo, dod = _g(B * Tq, HD, HD + 12, data=do)
    go, od = _g(B * Tq, HD, HD + 4, fill=NAN)
    md = None if mask is None else mask.to(DEV).contiguous()
    need = 2 * B * H * Tq * Tk * 4
    gs = R.Guard(32 + need + 32, 0xFF, torch.uint8, DEV)
    scratch = gs.view(32, (need,), (1,))
    for t in (gin, gout, gdo, go, gs):
        t.seal()
    a = L.AttentionArgs()
    a.B, a.H, a.Tq, a.Tk, a.head_dim, a.dtype = B, H, Tq, Tk, 64, L.SPRC_F32
    a.q, a.ldq, a.k, a.ldk, a.v, a.ldv, a.out, a.ldo = qd.data_ptr(), ld, kd.data_ptr(), ld, vd.data_ptr(), ld, od.data_ptr(), HD + 4
    a.key_mask, a.scale = (None if md is None else md.data_ptr()), scale
    b = L.AttentionBwdArgs()
    b.B, b.H, b.Tq, b.Tk, b.head_dim = B, H, Tq, Tk, 64
    b.q, b.k, b.v, b.dout, b.ldq, b.ldk, b.ldv, b.lddo = qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), dod.data_ptr(), ld, ld, ld, HD + 12
    b.key_mask, b.scale = a.key_mask, scale
    b.dq, b.dk, b.dv, b.lddq, b.lddk, b.lddv = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ld, ld, ld
    b.scratch, b.scratch_bytes = scratch.data_ptr(), need
    if drop is not None:
        a.drop_p, a.drop_seed, a.drop_site = drop
        b.drop_p, b.drop_seed, b.drop_site = drop
    _ok(lib.sprc_attention(C.byref(a), _st()), "sprc_attention")
    _ok(lib.sprc_attention_bwd(C.byref(b), _st()), "sprc_attention_bwd")
    tag = f"attention{tag} B={B} H={H} Tq={Tq} Tk={Tk} mask={int(mask is not None)} drop={int(drop is not None)}"
    R.calibrated(tag + " out", od, o64, o32, "attention (fp32 forward): out")
    for name, got, w64, w32 in zip(("dq", "dk", "dv"), (dq, dk, dv), g64, g32):
        R.calibrated(f"{tag} {name}", got, w64, w32, "attention_bwd: " + name)
    assert all(t.outside_intact() for t in (gout, go, gs)) and gin.outside_intact(whole=True) and gdo.outside_intact(whole=True), tag


def _key_mask(B, Tk, variant):
    """B = 2: batch 0 with EVERY key at -10000, batch 1 with a masked tail; B = 1: a masked tail, or none"""
    m = torch.zeros(B, Tk)
    if B == 2:
        m[0] = -10000.0
        m[1, Tk - Tk // 3:] = -10000.0
        return m
    if variant:
        m[0, Tk - Tk // 3:] = -10000.0
        return m
    return None


@gpu
@pytest.mark.parametrize("Tk", [1, 63, 64, 65, 257, 576])
def test_attention_fwd_and_bwd_packed_masked_with_and_without_dropout(Tk):
    for Tq, H, B in itertools.product((1, 3, 32), (1, 3), (1, 2)):              # B H Tq = 1 included: three of the four waves are dead
        mask = _key_mask(B, Tk, Tq == 3)
        _attn_case(B, H, Tq, Tk, mask, None)
        _attn_case(B, H, Tq, Tk, mask, (0.1, 0x9E3779B97F4A7C15 + Tk, 256 * 2 + 8 * 5 + 2))


@gpu
def test_attention_with_logits_of_sixty():
    """q and k scaled so that q k^T / 8 has a standard deviation of 14: over these 2 x 3 x 32 x 257 logits that spans about +-60"""
    _attn_case(2, 3, 32, 257, None, None, qk_scale=14.0 ** 0.5, tag="(+-60)")
    _attn_case(2, 3, 32, 257, None, (0.1, 77, 3), qk_scale=14.0 ** 0.5, tag="(+-60)")


# ---- 6. Q-Former embedding rows and their scatter -------------------------------------------------------------------------------------
def _embed_case(B, Lq, Lt, hidden, vocab, no_img, qstride, ids, tag, null_text=False):
    """qstride: 0 (one query block for the whole batch: dquery summed over it), or the elements between samples (>= Lq hidden)"""
    lib = L.load()
    S, shared = Lq + Lt, qstride == 0
    g = _gen(7, B, Lq, Lt, hidden, no_img, qstride)
    nq = 1 if shared else B
    query, word, pos = _rn(g, nq, Lq, hidden), _rn(g, vocab, hidden), _rn(g, S, hidden)
    dpre = _rn(g, B, S, hidden)
    init = [_rn(g, nq, Lq, hidden), _rn(g, vocab, hidden), _rn(g, S, hidden)]
    fn = R.embed_rows(ids, B, Lq, Lt, vocab, no_img, shared)
    qin = query[0] if shared else query
    pre64, g64 = R.grads_of(fn, [qin, word, pos], dpre, torch.float64)
    _, gabs = R.grads_of(fn, [qin, word, pos], dpre.abs(), torch.float64)
    _, cnt = R.grads_of(fn, [qin, word, pos], torch.ones_like(dpre), torch.float64)
    pre32 = fn(qin, word, pos)
    row = Lq * hidden
    ldq = max(qstride, row)
    gq, qd = _g(nq, row, ldq, data=query)
    gdq, dqd = _g(nq, row, ldq, data=init[0])
    gw, wd = _g(vocab, hidden, hidden, data=word)
    gdw, dwd = _g(vocab, hidden, hidden, data=init[1])
    gp, pd = _g(S, hidden, hidden, data=pos)
    gdp, dpd = _g(S, hidden, hidden, data=init[2])
    gpre, pred = _g(B * S, hidden, hidden, fill=NAN)
    gd, dd = _g(B * S, hidden, hidden, data=dpre)
    idd = None if null_text else ids.to(DEV).contiguous()
    guards_out, guards_in = (gdq, gdw, gdp, gpre), (gq, gw, gp, gd)
    for t in guards_out + guards_in:
        t.seal()
    a = L.QformerEmbedArgs()
    a.B, a.Lq, a.Lt, a.hidden, a.out_dtype, a.vocab, a.no_img = B, Lq, Lt, hidden, L.SPRC_F32, vocab, int(no_img)
    a.query_embeds, a.q_bstride = qd.data_ptr(), qstride
    if not null_text:
        a.input_ids, a.word_emb, a.pos_emb = idd.data_ptr(), wd.data_ptr(), pd.data_ptr()
    _ok(lib.sprc_qformer_embed_rows(C.byref(a), pred.data_ptr(), _st()), "sprc_qformer_embed_rows")
    _ok(lib.sprc_qformer_embed_bwd(C.byref(a), dd.data_ptr(), dqd.data_ptr(), qstride, None if null_text else dwd.data_ptr(),
                                   None if null_text else dpd.data_ptr(), _st()), "sprc_qformer_embed_bwd")
    torch.cuda.synchronize()
    assert torch.equal(_bits(pred.view(B, S, hidden)), _bits(pre32)), tag       # one fp32 add per element: bit-exact
    assert float((pre32.double() - pre64).abs().max()) <= 2.0 ** -23 * float(pre64.abs().max())
    for name, got, i in (("dquery", dqd, 0), ("dword", dwd, 1), ("dpos", dpd, 2)):
        i0 = init[i].double().reshape(g64[i].shape)
        R.assert_sum_bound(f"{tag} {name}", got.reshape(g64[i].shape), i0 + g64[i], cnt[i] + 1, i0.abs() + gabs[i])
    assert all(t.outside_intact() for t in guards_out) and all(t.outside_intact(whole=True) for t in guards_in), tag


@gpu
@pytest.mark.parametrize("hidden", [4, 64])
@pytest.mark.parametrize("no_img", [False, True])
def test_embedding_rows_and_scatter(hidden, no_img):
    B, Lq, Lt, vocab = 3, 3, 5, 50
    g = _gen(8, hidden, no_img)
    rand = torch.randint(0, vocab, (B, Lt), generator=g)
    same = torch.full((B, Lt), 7)                                               # one id in every position of every sample: every add collides
    edge = rand.clone()
    edge[:, 0], edge[:, -1], edge[1, 2] = -1, vocab, vocab + 1000               # clamped to 0 / vocab - 1, forward and backward alike
    for qstride in (0, Lq * hidden, Lq * hidden + 8):
        for name, ids in (("random", rand), ("repeated", same), ("clamped", edge)):
            _embed_case(B, Lq, Lt, hidden, vocab, no_img, qstride, ids, f"embed hidden={hidden} no_img={int(no_img)} q_bstride={qstride} ids={name}")
    if not no_img:                                                              # the target-image pass: query rows only, NULL text pointers
        for qstride in (0, Lq * hidden):
            _embed_case(B, Lq, 0, hidden, vocab, False, qstride, None, f"embed hidden={hidden} Lt=0 q_bstride={qstride}", null_text=True)


@gpu
def test_embedding_scatter_beyond_the_grid_cap_with_colliding_rows():
    B, Lq, Lt, hidden, vocab = 24, 32, 32, 768, 50
    assert B * (Lq + Lt) * hidden > GRID_CAP
    ids = torch.randint(0, vocab, (B, Lt), generator=_gen(9))
    _embed_case(B, Lq, Lt, hidden, vocab, False, 0, ids, "embed B=24 S=64 hidden=768")


# ---- 7. similarity maximum, backward --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B,N", [(1, 1), (5, 8), (6, 6)])
@pytest.mark.parametrize("J", [1, 32])
@pytest.mark.parametrize("E", [64, 100, 256])
def test_sim_max_bwd_first_argmax_and_accumulation(B, N, J, E):
    lib = L.load()
    g = _gen(10, B, N, J, E)
    base = _rn(g, E)
    fusion = F.normalize(base + 0.3 * _rn(g, B, E), dim=-1)                    # a common direction, so that one token can win for EVERY query
    feats = F.normalize(_rn(g, N, J, E), dim=-1)
    pairs = {}
    if J == 32:                                                                 # exact ties: token rows duplicated, placed AT the maximum
        for n in range(N):
            first, second = ((3, 17), (0, 31))[n % 2]
            feats[n, first] = feats[n, second] = F.normalize(base + 0.1 * _rn(g, E), dim=-1)
            pairs[n] = (first, second)
    dsim = _rn(g, B, N)
    dfu0, dfe0 = _rn(g, B, E), _rn(g, N, J, E)
    s = torch.einsum("be,nje->bnj", fusion.double(), feats.double())
    for n, (first, second) in pairs.items():
        s[:, n, second] = s[:, n, first]                                        # identical rows: one value (a blocked fp64 product may differ in the last bit by position)
    jref = R.first_argmax(s)
    s2 = s.clone()
    for n, (first, second) in pairs.items():
        s2[:, n, second] = -float("inf")                                        # the gap that must be clear is the one to the OTHER tokens
    top = s2.topk(min(2, J), dim=-1).values
    clear = torch.ones(B, N, dtype=torch.bool) if J == 1 else (top[..., 0] - top[..., 1]) > 1e-5
    for n, (first, second) in pairs.items():
        assert bool((jref[:, n] == first).all())                                # the duplicated pair IS the maximum, the reference takes its first
    assert bool(clear.all())
    onehot = F.one_hot(jref, J).double()                                        # [B, N, J]
    w = dsim.double()[..., None] * onehot
    dfu = dfu0.double() + torch.einsum("bnj,nje->be", w, feats.double())
    dfu_abs = dfu0.double().abs() + torch.einsum("bnj,nje->be", w.abs(), feats.double().abs())
    dfe = dfe0.double() + torch.einsum("bnj,be->nje", w, fusion.double())
    dfe_abs = dfe0.double().abs() + torch.einsum("bnj,be->nje", w.abs(), fusion.double().abs())
    gfu, fud = _g(1, B * E, B * E, data=fusion)
    gfe, fed = _g(1, N * J * E, N * J * E, data=feats)
    gds, dsd = _g(1, B * N, B * N, data=dsim)
    gdfu, dfud = _g(1, B * E, B * E, data=dfu0)
    gdfe, dfed = _g(1, N * J * E, N * J * E, data=dfe0)
    gj, jd = _g(1, B * N, B * N, fill=-7, dtype=torch.int32)
    for t in (gfu, gfe, gds, gdfu, gdfe, gj):
        t.seal()
    _ok(lib.sprc_sim_max_bwd(fud.data_ptr(), fed.data_ptr(), dsd.data_ptr(), B, N, J, E, dfud.data_ptr(), dfed.data_ptr(), jd.data_ptr(), _st()),
        "sprc_sim_max_bwd")
    torch.cuda.synchronize()
    got_j = jd.cpu().view(B, N).long()
    assert torch.equal(got_j[clear], jref[clear]), (got_j, jref)
    tag = f"sim_max_bwd B={B} N={N} J={J} E={E}"
    R.assert_sum_bound(tag + " dfusion", dfud.view(B, E), dfu, N + 1, dfu_abs)
    R.assert_sum_bound(tag + " dfeats", dfed.view(N, J, E), dfe, B + 1, dfe_abs)
    got_fe = dfed.cpu().view(N, J, E)
    for n, (first, second) in pairs.items():                                    # the whole gradient went to the first of the pair
        assert torch.equal(got_fe[n, second], dfe0[n, second])
    assert all(t.outside_intact() for t in (gdfu, gdfe, gj)) and all(t.outside_intact(whole=True) for t in (gfu, gfe, gds))


# ---- 8. contrastive cross entropy -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 200])
@pytest.mark.parametrize("temp", [1.0, 0.07, 0.01])
def test_contrastive_ce_forward_and_backward(B, temp):
    lib = L.load()
    g = _gen(11, B)
    sim = torch.rand((B, B), generator=g) * 2 - 1
    grad, dt0 = 2.5, 0.37
    fn = R.contrastive_ce()
    tt = torch.tensor(temp)
    l64, (ds64, dt64) = R.grads_of(fn, [sim, tt], torch.tensor(grad), torch.float64)
    l32, (ds32, dt32) = R.grads_of(fn, [sim, tt], torch.tensor(grad), torch.float32)
    gs, sd = _g(B, B, B + 3, data=sim)
    gl, ld_ = _g(1, 1, 1, fill=NAN)
    gds, dsd = _g(1, B * B, B * B, fill=NAN)
    gdt, dtd = _g(1, 1, 1, data=torch.tensor([dt0]))
    for t in (gs, gl, gds, gdt):
        t.seal()
    _ok(lib.sprc_contrastive_ce(sd.data_ptr(), B + 3, B, temp, ld_.data_ptr(), _st()), "sprc_contrastive_ce")
    _ok(lib.sprc_contrastive_ce_bwd(sd.data_ptr(), B + 3, B, temp, grad, dsd.data_ptr(), dtd.data_ptr(), _st()), "sprc_contrastive_ce_bwd")
    tag = f"contrastive_ce B={B} temp={temp}"
    if B == 1:
        torch.cuda.synchronize()
        assert float(ld_) == 0.0 and float(dsd) == 0.0
    R.calibrated(tag + " loss", ld_, l64, l32, "contrastive_ce: loss")
    R.calibrated(tag + " dsim", dsd, ds64, ds32, "contrastive_ce_bwd: dsim")
    R.calibrated(tag + " dtemp", dtd, dt0 + dt64, torch.tensor(dt0) + dt32, "contrastive_ce_bwd: dtemp")
    first = dsd.clone()
    gds.seal()
    _ok(lib.sprc_contrastive_ce_bwd(sd.data_ptr(), B + 3, B, temp, grad, dsd.data_ptr(), None, _st()), "sprc_contrastive_ce_bwd")     # dtemp = NULL
    torch.cuda.synchronize()
    assert torch.equal(_bits(dsd), _bits(first))
    assert all(t.outside_intact() for t in (gl, gds, gdt)) and gs.outside_intact(whole=True)


# ---- 9. L2 normalisation, backward ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M", [1, 3, 4, 5])
def test_l2norm_bwd(M):
    lib = L.load()
    for D in (1, 63, 64, 65, 256, 768):
        g = _gen(12, M, D)
        x, dy = _rn(g, M, D), _rn(g, M, D)
        zero_row = 1 if M == 3 else None
        if zero_row is not None:
            x[zero_row] = 0.0                                                  # max(||x||, 1e-12) clamps: dx = dy * 1e12, as F.normalize gives
        _, (dx64,) = R.grads_of(R.l2norm, [x], dy, torch.float64)
        _, (dx32,) = R.grads_of(R.l2norm, [x], dy, torch.float32)
        gx, xd = _g(M, D, D + 1, data=x)
        gdy, dyd = _g(M, D, D + 2, data=dy)
        gdx, dxd = _g(M, D, D + 3, fill=NAN)
        for t in (gx, gdy, gdx):
            t.seal()
        _ok(lib.sprc_l2norm_bwd(xd.data_ptr(), D + 1, dyd.data_ptr(), D + 2, dxd.data_ptr(), D + 3, M, D, _st()), "sprc_l2norm_bwd")
        live = [r for r in range(M) if r != zero_row]
        # dx = (dy - y <y, dy>) / ||x|| is a difference (for D = 1 it cancels to exactly 0): the floor of the bar is half an ulp of the
        # TERMS, max |dy| / ||x||, not of the result
        terms = float((dy[live].double().abs().amax(1) / x[live].double().norm(dim=1)).max())
        R.calibrated(f"l2norm_bwd M={M} D={D}", dxd[live], dx64[live], dx32[live], "l2norm_bwd: dx", scale=terms)
        if zero_row is not None:                                                # its own comparison: relative to ITS max|ref| (1e12 x the others')
            assert torch.allclose(dx64[zero_row], dy[zero_row].double() * 1e12, rtol=1e-12, atol=0)
            R.calibrated(f"l2norm_bwd M={M} D={D} zero row", dxd[zero_row], dx64[zero_row], dx32[zero_row], "l2norm_bwd: dx (zero row)")
        assert gdx.outside_intact() and gx.outside_intact(whole=True) and gdy.outside_intact(whole=True)


# ---- 10. alignment loss ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("D", [1, 255, 256, 257, 768])
def test_align_mse_forward_and_backward(D):
    lib = L.load()
    for Lq, B in itertools.product((1, 32), (1, 4)):
        g = _gen(13, D, Lq, B)
        h, prompt, dh0 = _rn(g, B, Lq, D), _rn(g, Lq, D), _rn(g, B, Lq, D)
        grad = 0.4
        s_h, s_d = (Lq + 2) * D + 4 * (1 + D % 4), (Lq + 3) * D + 4             # two sentinel rows j >= Lq behind every sample; s_h % 4 == 0 when D % 4 == 0
        l64, (dh64, _) = R.grads_of(R.align_mse, [h, prompt], torch.tensor(grad), torch.float64)
        l32 = R.align_mse(h, prompt)
        gh, hd = _g(B, Lq * D, s_h, data=h)
        gp, pd = _g(1, Lq * D, Lq * D, data=prompt)
        gdh, dhd = _g(B, Lq * D, s_d, data=dh0)
        gl, ld_ = _g(1, 1, 1, fill=NAN)
        for t in (gh, gp, gdh, gl):
            t.seal()
        tag = f"align_mse D={D} Lq={Lq} B={B}"
        rc = lib.sprc_align_mse(hd.data_ptr(), s_h, Lq, D, pd.data_ptr(), B, ld_.data_ptr(), _st())
        if D % 4 == 0:                                                          # the forward reads float4 rows: it serves D % 4 == 0 only ...
            _ok(rc, "sprc_align_mse")
            R.calibrated(tag + " loss", ld_, l64, l32, "align_mse: loss")
        else:                                                                   # ... and refuses the rest before any launch; the backward takes any D
            _refused(rc, b"unsupported")
        _ok(lib.sprc_align_mse_bwd(hd.data_ptr(), s_h, Lq, D, pd.data_ptr(), B, grad, dhd.data_ptr(), s_d, _st()), "sprc_align_mse_bwd")
        # dh[b, j, d] = dh0 + c (sum_j h[b, j, d] - sum_j prompt[j, d]), c = grad 2 / (B D Lq^2): 2 Lq terms + dh0, and five more roundings in
        # forming c and the two means -- counted as terms
        c = grad * 2.0 / (B * D * Lq * Lq)
        tabs = dh0.double().abs() + c * (h.double().abs().sum(1, keepdim=True) + prompt.double().abs().sum(0)[None, None, :])
        R.assert_sum_bound(tag + " dh", dhd.view(B, Lq, D), dh0.double() + dh64, 2 * Lq + 1 + 5, tabs.expand(B, Lq, D))
        assert gdh.outside_intact() and gl.outside_intact() and gh.outside_intact(whole=True) and gp.outside_intact(whole=True), tag


# ---- 11. dropout ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_dropout_beyond_the_grid_cap_with_residual_and_in_place():
    lib = L.load()
    n, seed, site, p = GRID_CAP + 5, 0xFEDCBA9876543210, 2 * 256 + 255, 0.1
    g = _gen(14)
    x, r = _rn(g, n), _rn(g, n)
    keep = R.keep_mask(seed, site, (n,), p)
    sc = torch.tensor(R.drop_scale(p), dtype=torch.float32)
    dropped = torch.where(keep, x * sc, torch.zeros(()))                        # one fp32 multiply: exact
    gx, xd = _g(1, n, n, data=x)
    gr, rd = _g(1, n, n, data=r)
    gy, yd = _g(1, n, n, fill=NAN)
    for t in (gx, gr, gy):
        t.seal()
    _ok(lib.sprc_dropout_f32(xd.data_ptr(), rd.data_ptr(), yd.data_ptr(), n, seed, site, p, _st()), "sprc_dropout_f32")
    torch.cuda.synchronize()
    want = dropped.double() + r.double()                                        # multiply, then add (possibly fused): within one ulp each
    err = (yd.cpu()[0].double() - want).abs()
    assert bool((err <= 2.0 ** -23 * (want.abs() + dropped.double().abs())).all())
    assert torch.equal(yd.cpu()[0][~keep], r[~keep])                            # the mask itself: dropped elements are the residual, bit for bit
    assert gy.outside_intact() and gx.outside_intact(whole=True) and gr.outside_intact(whole=True)
    # x aliasing y, no residual
    _ok(lib.sprc_dropout_f32(xd.data_ptr(), None, xd.data_ptr(), n, seed, site, p, _st()), "sprc_dropout_f32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(xd[0]), _bits(dropped)) and gx.outside_intact()
    assert torch.equal(xd.cpu()[0] != 0, keep & (x != 0))


# ---- 12. the linear layer's backward ------------------------------------------------------------------------------------------------------------
def _r16(half):
    return (lambda t: t.half().double()) if half else (lambda t: t.double())


@gpu
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("N,K", [(32, 64), (96, 160), (256, 768)])
def test_linear_bwd_against_autograd(half, N, K):
    """train._Linear.bwd: dW += dY^T X through zero-padded transposed operand copies, db += colsum(dY), dX (+ acc) = dY W.  half: the
    reference multiplies the fp16-ROUNDED operands in fp64, so that only accumulation error is left.  N = 32 and N = 96 in half mode
    are not multiples of the 16-bit K-tile (64): dX reduces over zero-padded columns there."""
    from sprc_amd import train as T
    r = _r16(half)
    ktile = 64 if half else 32
    for M in (1, 31, 33, 64, 123):
        g = _gen(15, half, N, K, M)
        k = T._K(torch.device(DEV), half=half)
        W, b, x, dy, x2 = _rn(g, N, K) * 0.1, _rn(g, N), _rn(g, M, K), _rn(g, M, N), _rn(g, M, K)
        gW0, gb0, acc0 = _rn(g, N, K), _rn(g, N), _rn(g, M, K)
        _, (dx64, dW64, _) = R.grads_of(F.linear, [r(x), r(W), b], r(dy), torch.float64)
        dW_abs, dx_abs = r(dy).abs().t() @ r(x).abs(), r(dy).abs() @ r(W).abs()
        db64, db_abs = dy.double().sum(0), dy.double().abs().sum(0)
        dev = lambda *ts: [t.to(DEV).clone() for t in ts]                       # noqa: E731
        xd, dyd, x2d = dev(x, dy, x2)
        tag = f"linear half={int(half)} M={M} N={N} K={K}"
        # _K.transpose: zero-padded transposed operand copy
        xt = k.transpose(xd)
        mp = (M + ktile - 1) // ktile * ktile
        assert xt.shape == (K, mp) and torch.equal(_bits(xt[:, :M]), _bits(x.t().half() if half else x.t())) and not bool(xt[:, M:].any())
        # _K.gemm: y = x W^T + b (the forward product needs K a multiple of the K-tile; the other K is refused, not mangled)
        P = dict(zip(("w", "b"), dev(W, b)))
        if K % ktile == 0:
            y = k.gemm(xd, P["w"], bias=P["b"])
            y64 = F.linear(r(x), r(W), b.double())
            R.assert_sum_bound(tag + " y", y, y64, K + 1, r(x).abs() @ r(W).abs().t() + b.double().abs())
        else:
            with pytest.raises(L.SprcError, match="multiple of"):
                k.gemm(xd, P["w"], bias=P["b"])
        # with bias, acc given; twice on the same layer: W^T is formed once, the gradients add
        G = dict(zip(("w", "b"), dev(gW0, gb0)))
        lin = T._Linear(k, P, G, "w", "b")
        acc = acc0.to(DEV).clone()
        out = lin.bwd(xd, dyd, acc=acc)
        assert out is acc and lin._Wt is not None and lin._Wt.shape[1] % ktile == 0
        R.assert_sum_bound(tag + " dW", G["w"], gW0.double() + dW64, M + 1, gW0.double().abs() + dW_abs)
        R.assert_sum_bound(tag + " db", G["b"], gb0.double() + db64, M + 1, gb0.double().abs() + db_abs)
        R.assert_sum_bound(tag + " dx+acc", out, acc0.double() + dx64, N + 1, acc0.double().abs() + dx_abs)
        wt = lin._Wt
        out2 = lin.bwd(xd, dyd)                                                 # acc not given: a fresh dx
        assert lin._Wt is wt and out2 is not acc
        R.assert_sum_bound(tag + " dW (2nd call)", G["w"], gW0.double() + 2 * dW64, 2 * M + 1, gW0.double().abs() + 2 * dW_abs)
        R.assert_sum_bound(tag + " db (2nd call)", G["b"], gb0.double() + 2 * db64, 2 * M + 1, gb0.double().abs() + 2 * db_abs)
        R.assert_sum_bound(tag + " dx", out2, dx64, N, dx_abs)
        # without bias, need_dx = False: no W^T is formed, dW still accumulates
        G2 = {"w": gW0.to(DEV).clone()}
        lin2 = T._Linear(k, P, G2, "w", None)
        assert lin2.bwd(xd, dyd, need_dx=False) is None and lin2._Wt is None and lin2.gb is None
        R.assert_sum_bound(tag + " dW (no bias, no dx)", G2["w"], gW0.double() + dW64, M + 1, gW0.double().abs() + dW_abs)
        # transpose_saved: two inputs with several consumers each; the last consumer of each empties the cache
        assert len(k._xt) == 0
        lin2.bwd(xd, dyd, need_dx=False, shared=1)
        lin2.bwd(x2d, dyd, need_dx=False, shared=1)
        assert len(k._xt) == 2
        lin2.bwd(xd, dyd, need_dx=False, shared=2)
        assert len(k._xt) == 1 and id(x2d) in k._xt
        lin2.bwd(x2d, dyd, need_dx=False, shared=2)
        assert len(k._xt) == 0
        dW2 = r(dy).t() @ r(x2)
        R.assert_sum_bound(tag + " dW (shared)", G2["w"], gW0.double() + 3 * dW64 + 2 * dW2, 5 * M + 1,
                           gW0.double().abs() + 3 * dW_abs + 2 * (r(dy).abs().t() @ r(x2).abs()))


# ---- refusals: before any launch, so these run without a GPU ------------------------------------------------------------------------------------
def test_refusals_need_no_launch():
    """Every pointer below is a dummy that is never dereferenced: each call is refused (or, for n = 0, accepted) before any launch."""
    lib = L.load()
    p = [0x10000 * (i + 1) for i in range(8)]                                   # 16-byte aligned dummies
    # transposes: a dtype that is not 16-bit
    _refused(lib.sprc_transpose_f32_to16(p[0], 8, p[1], 8, 4, 4, L.SPRC_F32, None), b"16-bit")
    _refused(lib.sprc_transpose_f32_to16(p[0], 8, p[1], 8, 4, 4, L.SPRC_FP8, None), b"16-bit")
    _refused(lib.sprc_transpose_f32(p[0], 3, p[1], 8, 4, 4, None))              # ld_src < cols
    _refused(lib.sprc_colsum_f32(p[0], 3, 4, 4, p[1], 0, None))                 # ld < N
    # gelu: n = 0 is OK without a launch
    assert lib.sprc_gelu_fwd(p[0], p[1], 0, None) == 0 and lib.sprc_gelu_bwd(p[0], p[1], p[2], 0, None) == 0
    _refused(lib.sprc_gelu_fwd(None, p[1], 4, None), b"null")
    # LayerNorm backward
    need = int(lib.sprc_layernorm_bwd_workspace_bytes(33, 256))
    assert need == 2 * 2 * 256 * 4

    def ln(D=256, ldx=260, ws=p[6], ws_bytes=need, M=33):
        return lib.sprc_layernorm_bwd(p[0], ldx, p[1], p[2], 264, 1e-5, M, D, p[3], 268, p[4], p[5], ws, ws_bytes, None)
    _refused(ln(D=2052, ldx=2056, ws_bytes=1 << 20), b"unsupported")
    _refused(ln(D=6, ldx=8), b"unsupported")
    _refused(ln(ldx=261), b"unsupported")
    _refused(ln(ws_bytes=need - 1), b"workspace")
    _refused(ln(ws=p[6] + 4), b"workspace")
    # attention backward
    b = L.AttentionBwdArgs()
    b.B, b.H, b.Tq, b.Tk, b.head_dim = 2, 3, 4, 576, 64
    b.q, b.k, b.v, b.dout, b.dq, b.dk, b.dv, b.scratch = p
    b.ldq = b.ldk = b.ldv = b.lddo = b.lddq = b.lddk = b.lddv = 192
    b.scale, b.scratch_bytes = 0.125, 2 * 2 * 3 * 4 * 576 * 4
    for field, value, word in (("Tk", 577, b"Tk=577"), ("head_dim", 72, b"head_dim"), ("scratch_bytes", b.scratch_bytes - 1, b"scratch"),
                               ("drop_p", 1.0, b"drop_p")):
        keep = getattr(b, field)
        setattr(b, field, value)
        _refused(lib.sprc_attention_bwd(C.byref(b), None), word)
        setattr(b, field, keep)
    # dropout: p outside [0, 1)
    _refused(lib.sprc_dropout_f32(p[0], None, p[1], 16, 1, 2, 1.0, None), b"outside")
    _refused(lib.sprc_dropout_f32(p[0], None, p[1], 16, 1, 2, -0.1, None), b"outside")
    # embeddings: the text-only layout needs a first token; the backward makes the forward's shape checks
    a = L.QformerEmbedArgs()
    a.B, a.Lq, a.Lt, a.hidden, a.out_dtype, a.vocab, a.no_img = 2, 3, 4, 8, L.SPRC_F32, 50, 0
    a.query_embeds, a.q_bstride, a.input_ids, a.word_emb, a.pos_emb = p[0], 0, p[1], p[2], p[3]

    def both(word):
        _refused(lib.sprc_qformer_embed_rows(C.byref(a), p[4], None), word)
        _refused(lib.sprc_qformer_embed_bwd(C.byref(a), p[4], p[5], 0, p[6], p[7], None), word)
    for field, value in (("B", 0), ("Lq", -1), ("Lt", -1), ("hidden", 0), ("hidden", -4)):
        keep = getattr(a, field)
        setattr(a, field, value)
        both(b"bad shape")
        setattr(a, field, keep)
    a.Lq, a.Lt = 0, 0
    both(b"bad shape")
    a.Lq, a.Lt, a.no_img = 3, 0, 1                                              # row 0 would read input_ids[b * Lt]: there is no token
    a.input_ids = a.word_emb = a.pos_emb = None
    both(b"no_img needs Lt >= 1")
    a.input_ids, a.word_emb, a.pos_emb = p[1], p[2], p[3]
    both(b"no_img needs Lt >= 1")
    a.Lt, a.no_img, a.input_ids = 4, 0, None
    both(None)                                                                  # text rows without ids: refused by both (each in its own words)
    a.input_ids = p[1]
    _refused(lib.sprc_qformer_embed_bwd(C.byref(a), None, p[5], 0, p[6], p[7], None), b"null")
    _refused(lib.sprc_qformer_embed_bwd(C.byref(a), p[4], p[5], 0, None, p[7], None), b"dword")
    a.hidden = 6
    _refused(lib.sprc_qformer_embed_rows(C.byref(a), p[4], None), b"bad shape")
    # heads and losses
    _refused(lib.sprc_sim_max_bwd(p[0], p[1], p[2], 2, 2, 0, 64, p[3], p[4], p[5], None))
    _refused(lib.sprc_contrastive_ce_bwd(p[0], 3, 4, 0.07, 1.0, p[1], None, None))          # ld < B
    _refused(lib.sprc_contrastive_ce_bwd(p[0], 4, 4, 0.0, 1.0, p[1], None, None))           # temp = 0
    _refused(lib.sprc_l2norm_bwd(p[0], 4, p[1], 4, None, 4, 2, 4, None))
    _refused(lib.sprc_align_mse_bwd(p[0], 64, 0, 4, p[1], 2, 1.0, p[2], 64, None))
    _refused(lib.sprc_align_mse(p[0], 1028, 4, 255, p[1], 2, p[2], None), b"unsupported")


@gpu
def test_zz_print_the_calibration_table():
    """Not a check of its own: prints the largest e_kernel / e_torch of this session per kernel output (the table of DESIGN.md 4.4)."""
    for key in sorted(R.RATIOS):
        print(f"[calibration] {key}: {R.RATIOS[key]:.2f}")
    assert all(v <= 4.0 for v in R.RATIOS.values())
