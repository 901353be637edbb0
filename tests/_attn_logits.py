"""Attention inputs with STRUCTURED softmax logits (tests/test_attention_range_gpu.py; checked on the host by tests/test_attn_logits.py).

N(0, 1) queries and keys with scale head_dim ** -0.5 give scores of about N(0, 1): after the first 32-key tile the running max of the
online softmax never moves, so the rescale code of the streaming kernels (sprc_amd/csrc/attention.hip: `tile` and `tail_small`, lazy
by RESCALE_LOG2 = 8 log2 units) and the fp16 range of P are never exercised.  Here every (batch, head, query) row gets a logit PATTERN
of its own -- rows of one 32-query tile disagree, so the wave-uniform `__any(...)` branches run with lanes on both sides.

Construction, per head (head_dim >= 16):
  * the first dims: noise -- N(0, 1) on the keys that are NOT locations, scaled on q to a score std of `sigma` nats;
  * one dim per LOCATION (a single key each: the tile-0 peak, a middle tile, the last full tile, the ragged last tile, the first and the
    last tile of a second key segment): k = K0 on that key only, q = logit / (scale K0);
  * dim RAMP:  k = KR * tile index (key // 32), q = step / (scale KR)   -> a staircase of `step` nats per 32-key tile;
  * dim CONST (the last): k = K0 for every key, q = offset / (scale K0)   -> adds `offset` nats to the whole row.
The large terms come last in the head, so a dot product accumulated in head order rounds at their magnitude once, not at every step.
The location keys carry no noise, so a row's tile-0 max and its late key are exactly the logits asked for (up to the 16-bit rounding of
q).  Everything is then recomputed in float64 from the operands the kernel receives (rounded to bf16 / fp16 where it takes those), and
`Case.scores` / `Case.tile_max` report what the construction actually produced.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

RESCALE_NATS = 8.0 * math.log(2.0)      # the streaming kernels move their running max when a tile's max exceeds it by more than this
TILE = 32
K0 = 16.0                               # key-side value of the location and offset dims, and KR per tile of the ramp (exact in every
KR = 4.0                                # dtype): the large products split between q and k keep the fp32 gradients through both small
MASK_VALUE = -10000.0                   # the header's key-mask contract: (1 - m) * -10000
JUMPS = (5.3, 5.8, 15.0, 40.0)          # just under / just over the threshold (5.545); past fp16's range of P were it above 16 log2; far past
GAPS = (3.0, 20.0, 60.0)
T0_KEY = 5                              # the tile-0 peak
LATE_BASE = 3.0                         # logit of the tile-0 peak in late-jump rows: above the noise (sigma 0.5) of tile 0
NOISE = 0.5


@dataclass(frozen=True)
class Pattern:
    name: str
    logits: Dict[str, float] = field(default_factory=dict)    # location -> logit (nats); locations not named: 0
    step: float = 0.0            # staircase nats per tile
    offset: float = 0.0          # added to every score of the row
    sigma: float = NOISE         # noise std of the non-location keys (nats)
    kind: str = "flat"           # flat | early | late | stair
    jump: float = 0.0            # late: nats above the tile-0 max
    loc: str = ""                # late: where the late key sits
    gap: float = 0.0             # early: nats between the tile-0 peak and the rest


def locations(Tk1: int, Tk2: int = 0) -> Dict[str, int]:
    """Key index of every location of a key axis cat(segment 1: Tk1 keys, segment 2: Tk2 keys)."""
    Tk = Tk1 + Tk2
    nkt = (Tk + TILE - 1) // TILE
    full = Tk // TILE                                     # whole tiles
    locs = {"t0": T0_KEY}
    last_full = full - 1
    if Tk2:
        locs["seg2_first"] = Tk1 + 2                       # in the tile where segment 2 starts
        locs["seg2_last"] = Tk - 1                         # the last key of segment 2 (and of the axis)
        mid = min(3, Tk1 // TILE - 1)
    else:
        mid = (nkt - 1) // 2
        if Tk % TILE:
            locs["tail"] = Tk - 1                          # the ragged last tile: tail_small when it holds <= 4 keys
    if 0 < mid < last_full:
        locs["mid"] = mid * TILE + 17
    if last_full > 0 and (Tk2 == 0 or last_full * TILE + 30 < Tk1 or last_full * TILE >= Tk1):
        locs["lastfull"] = last_full * TILE + 30
    return locs


def tail_kind(Tk: int) -> str:
    r = Tk % TILE
    return "none" if r == 0 else ("small" if r <= 4 else "generic")


def patterns(locs: Dict[str, int]) -> List[Pattern]:
    """Every row pattern this key axis supports (the late locations are those of `locs` other than the tile-0 peak)."""
    late = lambda loc, j, off=0.0: Pattern(f"late{j:g}@{loc}{off:+g}" if off else f"late{j:g}@{loc}",    # noqa: E731
                                           {"t0": LATE_BASE, loc: LATE_BASE + j}, offset=off, kind="late", jump=j, loc=loc)
    out = [Pattern("flat", sigma=1.0)]
    for g in GAPS:                                       # the max in tile 0, nothing moves after it
        out.append(Pattern(f"early{g:g}", {"t0": g + 3.0}, kind="early", gap=g))
    late_locs = [n for n in ("mid", "lastfull", "tail", "seg2_first", "seg2_last") if n in locs]
    for loc in late_locs:
        out += [late(loc, j) for j in JUMPS]
    # staircase: the tile max climbs by `step` per tile (noise 0.05 keeps each climb on its side of the threshold)
    out.append(Pattern("stair5", step=5.0, sigma=0.05, kind="stair"))
    out.append(Pattern("stair6", step=6.0, sigma=0.05, kind="stair"))
    # offsets: a softmax that failed to subtract its max over- / underflows here
    out.append(Pattern("early3+50", {"t0": 6.0}, offset=50.0, kind="early", gap=3.0))
    out.append(Pattern("flat-50", offset=-50.0, sigma=1.0))
    out.append(Pattern("stair6-50", step=6.0, sigma=0.05, offset=-50.0, kind="stair"))
    if late_locs:
        out += [late(late_locs[-1], 5.8, -50.0), late(late_locs[-1], 15.0, 50.0)]
    return out


MASKS = ("first_tile", "first_two_tiles", "peak_key", "one_key")


def make_mask(kind: str, Tk: int, locs: Dict[str, int]) -> torch.Tensor:
    """keep vector [Tk] (1 = attend) of a mask kind; every kind keeps at least one key."""
    keep = torch.ones(Tk)
    if kind == "first_tile":
        keep[:TILE] = 0
    elif kind == "first_two_tiles":
        keep[:2 * TILE] = 0
    elif kind == "peak_key":                               # the tile-0 peak and the middle tile's late key
        keep[locs["t0"]] = 0
        if "mid" in locs:
            keep[locs["mid"]] = 0
    elif kind == "one_key":
        keep[:] = 0
        keep[min(TILE + 8, Tk - 1)] = 1
    elif kind != "none":
        raise ValueError(kind)
    assert keep.sum() >= 1
    return keep


_TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}


@dataclass
class Case:
    B: int
    H: int
    Tq: int
    Tk1: int
    Tk2: int
    dh: int
    dtype: str
    scale: float                  # the fp32 value the kernel receives
    q: torch.Tensor               # [B, Tq, H, dh] in the kernel's dtype
    ka: torch.Tensor              # [NA, Tk1, H, dh] segment 1 bank (row ia[b] serves sample b)
    va: torch.Tensor
    kb: Optional[torch.Tensor]    # [NB, Tk2, H, dh] segment 2 bank
    vb: Optional[torch.Tensor]
    ia: Optional[torch.Tensor]    # int32 [B] or None (= b)
    ib: Optional[torch.Tensor]
    mask: Optional[torch.Tensor]  # fp32 [B, Tk] additive, or None
    mask_kinds: Optional[List[str]]
    locs: Dict[str, int]
    pats: List[Pattern]
    row_pat: torch.Tensor         # [B, H, Tq] index into pats

    @property
    def Tk(self) -> int:
        return self.Tk1 + self.Tk2

    def keys(self):
        """(k, v) of every sample's whole key axis [B, Tk, H, dh], float64 of the operands."""
        ia = torch.arange(self.B) if self.ia is None else self.ia.long()
        k, v = self.ka.double()[ia], self.va.double()[ia]
        if self.Tk2:
            ib = torch.arange(self.B) if self.ib is None else self.ib.long()
            k, v = torch.cat([k, self.kb.double()[ib]], 1), torch.cat([v, self.vb.double()[ib]], 1)
        return k, v

    @property
    def scores(self) -> torch.Tensor:
        """float64 [B, H, Tq, Tk]: scale * q . k from the operands, WITHOUT the mask"""
        k, _ = self.keys()
        return torch.einsum("bqhd,bkhd->bhqk", self.q.double(), k) * self.scale

    def logits(self) -> torch.Tensor:
        s = self.scores
        if self.mask is not None:
            s = s + self.mask.double()[:, None, None, :]
        return s

    def tile_max(self, s: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[B, H, Tq, n_tiles] max of each 32-key tile"""
        s = self.scores if s is None else s
        pad = (-s.shape[-1]) % TILE
        s = torch.nn.functional.pad(s, (0, pad), value=-math.inf)
        return s.view(*s.shape[:-1], -1, TILE).amax(-1)

    def reference(self) -> torch.Tensor:
        """float64 [B, Tq, H, dh] = softmax(scale q k^T + mask) v of the operands the kernel receives"""
        _, v = self.keys()
        p = torch.softmax(self.logits(), dim=-1)
        return torch.einsum("bhqk,bkhd->bqhd", p, v)

    def flat(self, t: torch.Tensor) -> torch.Tensor:
        """[N, T, H, dh] -> [N * T, H * dh] contiguous (the token-row layout of sprc_attention)"""
        return t.reshape(t.shape[0] * t.shape[1], t.shape[2] * t.shape[3]).contiguous()


def make_case(B: int, H: int, Tq: int, Tk1: int, dh: int, dtype: str, seed: int, Tk2: int = 0, ia=None, ib=None,
              NA: Optional[int] = None, NB: Optional[int] = None, masks: Optional[List[str]] = None) -> Case:
    """ia / ib: lists of bank rows per sample (None: sample b uses row b); masks: one kind of MASKS (or "none") per sample."""
    assert dh >= 16
    g = torch.Generator().manual_seed(seed)
    tdt = _TDT[dtype]
    scale = float(torch.tensor(dh ** -0.5, dtype=torch.float32))
    locs = locations(Tk1, Tk2)
    pats = patterns(locs)
    names = list(locs)
    nz = list(range(dh - 2 - len(names)))
    cdim = {n: len(nz) + i for i, n in enumerate(names)}
    RAMP, CONST = dh - 2, dh - 1
    NA = B if NA is None else NA
    NB = B if NB is None else NB

    def bank(N, T, first):
        k = torch.zeros(N, T, H, dh, dtype=torch.float64)
        k[..., CONST] = K0
        k[..., RAMP] = KR * (torch.arange(first, first + T) // TILE).double()[None, :, None]
        noise = torch.randn(N, T, H, len(nz), generator=g, dtype=torch.float64)
        for n in names:                                    # location keys: no noise, K0 in their own dim
            j = locs[n] - first
            if 0 <= j < T:
                noise[:, j] = 0.0
                k[:, j, :, cdim[n]] = K0
        k[..., nz] = noise
        v = torch.randn(N, T, H, dh, generator=g, dtype=torch.float64)
        return k.to(tdt), v.to(tdt)

    ka, va = bank(NA, Tk1, 0)
    kb, vb = bank(NB, Tk2, Tk1) if Tk2 else (None, None)
    # rows: pattern (i + 7 (b H + h)) mod len(pats) -- every tile of 32 rows holds all patterns, and short query axes see them across heads
    row_pat = (torch.arange(Tq)[None, None, :] + 7 * torch.arange(B * H).view(B, H, 1)) % len(pats)
    q = torch.zeros(B, Tq, H, dh, dtype=torch.float64)
    zq = torch.randn(B, Tq, H, len(nz), generator=g, dtype=torch.float64)
    zq = zq / zq.norm(dim=-1, keepdim=True)                # unit norm: the noise std of a row is its sigma
    for b in range(B):
        for h in range(H):
            for i in range(Tq):
                p = pats[int(row_pat[b, h, i])]
                q[b, i, h, CONST] = p.offset / (scale * K0)
                q[b, i, h, RAMP] = p.step / (scale * KR)
                for n, lg in p.logits.items():
                    q[b, i, h, cdim[n]] = lg / (scale * K0)
                q[b, i, h, nz] = zq[b, i, h] * (p.sigma / scale)
    q = q.to(tdt)
    mask = None
    if masks is not None:
        assert len(masks) == B and Tk2 == 0
        mask = torch.stack([(1.0 - make_mask(m, Tk1, locs)) * MASK_VALUE for m in masks]).float()
    t32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32)  # noqa: E731
    return Case(B, H, Tq, Tk1, Tk2, dh, dtype, scale, q, ka, va, kb, vb, t32(ia), t32(ib), mask, masks, locs, pats, row_pat)


# ---- the path matrix of tests/test_attention_range_gpu.py (sprc_amd/csrc/attention.hip: attention16 picks the kernel by shape) -------------
# path: the kernel the shape is meant to reach; dtypes: where it runs; kw: make_case arguments (B, H, Tq, Tk1, dh, ...); x3: fp16 also with
# the split-precision output rows
M4 = list(MASKS)
SPECS = [
    # streaming, one wave: Tq <= 32, Tk >= 128, head_dim <= 64, no mask, one segment (the Q-Former's cross-attention; kv_index = fuse_kv)
    ("stream1_q32_k256_kvidx", "stream1", ("bf16", "fp16"), dict(B=3, H=2, Tq=32, Tk1=256, dh=64, ia=[2, 0, 2], NA=3), True),
    ("stream1_q17_k256", "stream1", ("bf16", "fp16"), dict(B=2, H=3, Tq=17, Tk1=256, dh=64), True),
    ("stream1_q32_k257_kvidx", "stream1", ("bf16", "fp16"), dict(B=3, H=2, Tq=32, Tk1=257, dh=64, ia=[1, 1, 0], NA=2), True),
    ("stream1_q17_k257_kvidx", "stream1", ("bf16", "fp16"), dict(B=3, H=3, Tq=17, Tk1=257, dh=64, ia=[2, 0, 2], NA=3), True),
    ("stream1_q32_k261_kvidx", "stream1", ("bf16", "fp16"), dict(B=3, H=2, Tq=32, Tk1=261, dh=64, ia=[1, 2, 1], NA=3), True),
    ("stream1_q17_k261", "stream1", ("bf16", "fp16"), dict(B=2, H=3, Tq=17, Tk1=261, dh=64), True),
    # streaming, three waves: Tq > 128, no mask / segment / kv_index (the ViT blocks); head_dim 88 takes the denominator from a ones row
    ("stream3_dh64_k256", "stream3", ("bf16", "fp16"), dict(B=2, H=2, Tq=160, Tk1=256, dh=64), False),
    ("stream3_dh64_k257", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=257, Tk1=257, dh=64), False),
    ("stream3_dh64_k261", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=200, Tk1=261, dh=64), False),
    ("stream3_dh88_k256", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=256, Tk1=256, dh=88), False),
    ("stream3_dh88_k257", "stream3", ("bf16", "fp16"), dict(B=2, H=2, Tq=257, Tk1=257, dh=88), False),
    ("stream3_dh88_k261", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=161, Tk1=261, dh=88), False),
    ("stream3_dh72_k261", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=257, Tk1=261, dh=72), False),
    ("stream3_dh96_k257", "stream3", ("bf16", "fp16"), dict(B=1, H=2, Tq=257, Tk1=257, dh=96), False),
    # resident, nine waves: 257..288 queries with a key mask (the ViT-g shape under a mask)
    ("res9_dh64_masked", "res9", ("bf16", "fp16"), dict(B=4, H=2, Tq=257, Tk1=257, dh=64, masks=M4), False),
    ("res9_dh88_masked", "res9", ("bf16", "fp16"), dict(B=4, H=1, Tq=270, Tk1=261, dh=88, masks=M4), False),
    # resident, two waves: Tq <= 128, head_dim <= 64, at most 64 keys, masked (the Q-Former's self-attention: 32 queries + 24 text tokens)
    ("res2_q56_k56_masked", "res2", ("bf16", "fp16"), dict(B=3, H=2, Tq=56, Tk1=56, dh=64, masks=["first_tile", "peak_key", "one_key"]), False),
    # resident, four waves: Tq <= 128 over more than 64 keys (masked, or two 257-token segments with kv_index / kv2_index)
    ("res4_dh64_masked", "res4", ("bf16", "fp16"), dict(B=4, H=2, Tq=64, Tk1=257, dh=64, masks=M4), False),
    ("res4_dh96_masked", "res4", ("bf16", "fp16"), dict(B=4, H=2, Tq=32, Tk1=261, dh=96, masks=M4), False),
    ("res4_two_segments", "res4", ("bf16", "fp16"),
     dict(B=3, H=2, Tq=32, Tk1=257, Tk2=257, dh=64, ia=[1, 0, 1], ib=[2, 2, 0], NA=2, NB=3), False),
    # resident, eight waves: Tq > 128 but not nine query tiles, masked or two segments
    ("res8_dh64_masked", "res8", ("bf16", "fp16"), dict(B=4, H=1, Tq=200, Tk1=257, dh=64, masks=M4), False),
    ("res8_dh96_masked", "res8", ("bf16", "fp16"), dict(B=4, H=1, Tq=160, Tk1=261, dh=96, masks=M4), False),
    ("res8_two_segments", "res8", ("bf16", "fp16"), dict(B=2, H=2, Tq=150, Tk1=257, Tk2=257, dh=64, ia=[1, 0], ib=[0, 0], NA=2, NB=1), False),
    # the fp32 kernel (parity / training mode)
    ("f32_masked", "f32", ("f32",), dict(B=4, H=2, Tq=40, Tk1=261, dh=64, masks=M4), False),
    ("f32_dh88_masked", "f32", ("f32",), dict(B=4, H=1, Tq=33, Tk1=257, dh=88, masks=M4), False),
    ("f32_two_segments", "f32", ("f32",), dict(B=3, H=2, Tq=32, Tk1=257, Tk2=257, dh=64, ia=[1, 0, 1], ib=[2, 2, 0], NA=2, NB=3), False),
]
# the fp32 backward (sprc_attention_bwd: head_dim 64, one key segment, no kv_index)
BWD_SPECS = [
    ("bwd_masked", dict(B=4, H=2, Tq=32, Tk1=261, dh=64, masks=M4)),
    ("bwd_k257", dict(B=2, H=2, Tq=17, Tk1=257, dh=64)),
]


def check_case(c: Case) -> List[str]:
    """What went wrong in the construction of `c` (empty: every row came out as its pattern says), in float64 from the operands."""
    bad = []
    s = c.scores
    tm = c.tile_max(s)
    tile_of = lambda key: key // TILE                     # noqa: E731
    if not torch.isfinite(s).all():
        return ["non-finite scores"]
    for b in range(c.B):
        for h in range(c.H):
            kinds_per_tile = {}
            for i in range(c.Tq):
                p = c.pats[int(c.row_pat[b, h, i])]
                row, t = s[b, h, i], tm[b, h, i]
                where = f"b{b} h{h} q{i} {p.name}"
                kinds_per_tile.setdefault(i // TILE, set()).add((p.kind, p.jump > RESCALE_NATS))
                if p.offset and abs(float(t[0]) - p.offset) > 10.0:
                    bad.append(f"{where}: tile-0 max {float(t[0]):.2f} not near the offset {p.offset}")
                if p.kind == "early":
                    t0 = c.locs["t0"]
                    others = torch.cat([row[:t0], row[t0 + 1:]])
                    gap = float(row[t0] - others.max())
                    if not p.gap <= gap <= p.gap + 3.0:
                        bad.append(f"{where}: gap {gap:.3f}")
                elif p.kind == "late":
                    key = c.locs[p.loc]
                    jump = float(row[key] - t[0])
                    if int(row.argmax()) != key or float(t[0]) != float(row[c.locs["t0"]]):
                        bad.append(f"{where}: the max is not the late key / tile 0's max is not its peak")
                    if abs(jump - p.jump) > 0.1 + 0.005 * p.jump or abs(jump - RESCALE_NATS) < 0.15 or (jump > RESCALE_NATS) != (p.jump > RESCALE_NATS):
                        bad.append(f"{where}: jump {jump:.3f} nats (threshold {RESCALE_NATS:.3f})")
                    between = t[1:tile_of(key)] - t[0]      # (a lazy running max stays at tile 0's until the late key)
                    if between.numel() and float(between.max()) > 1.0:
                        bad.append(f"{where}: a tile before the late key rises above tile 0")
                elif p.kind == "stair":
                    d = t[1:] - t[:-1]
                    if float((d - p.step).abs().max()) > 0.3 or float((d - RESCALE_NATS).abs().min()) < 0.15 or \
                            bool(((d > RESCALE_NATS) != (p.step > RESCALE_NATS)).any()):
                        bad.append(f"{where}: tile climbs {[round(float(x), 2) for x in d]}")
            if c.Tq >= TILE:
                for qt, kinds in kinds_per_tile.items():
                    if (qt + 1) * TILE <= c.Tq and not ({("late", True), ("late", False)} <= kinds and ("early", False) in kinds):
                        bad.append(f"b{b} h{h} query tile {qt}: rows do not disagree on the rescale ({sorted(kinds)})")
    if c.mask is not None:
        lg = c.logits()
        ltm = c.tile_max(lg)
        for b, kind in enumerate(c.mask_kinds):
            keep = c.mask[b] == 0
            if int(keep.sum()) < 1:
                bad.append(f"b{b} {kind}: no key left")
            if kind in ("first_tile", "first_two_tiles"):
                n = TILE if kind == "first_tile" else 2 * TILE
                if bool(keep[:n].any()) or not bool(keep[n:].all()):
                    bad.append(f"b{b} {kind}: wrong keys masked")
                # the masked leading tile(s) set a running max near -10000 that the next tile replaces with alpha = 0
                if float(ltm[b, :, :, :n // TILE].max()) > -9000.0 or float(ltm[b, :, :, n // TILE:].max(-1).values.min()) < -200.0:
                    bad.append(f"b{b} {kind}: leading tiles not far below the rest")
            elif kind == "peak_key":
                if bool(keep[c.locs["t0"]]) or int(keep.sum()) != c.Tk - (2 if "mid" in c.locs else 1):
                    bad.append(f"b{b} {kind}: wrong keys masked")
            elif kind == "one_key":
                if int(keep.sum()) != 1:
                    bad.append(f"b{b} {kind}: {int(keep.sum())} keys kept")
    return bad


def case_for(sid: str, kw: dict, dtype: str) -> Case:
    """The case of spec `sid` in `dtype` (a fixed seed per spec and dtype: the host check and the GPU test draw the same inputs)."""
    return make_case(dtype=dtype, seed=zlib.crc32(f"{sid}/{dtype}".encode()) & 0x7FFFFFFF, **kw)


def expected_path(kw: dict, dtype: str) -> str:
    """The kernel attention16 / the fp32 branch of sprc_attention selects for a spec (a restatement of the dispatch in attention.hip,
    for the plain output layout: no key mask <=> kw has no `masks`)."""
    if dtype == "f32":
        return "f32"
    Tq, Tk, dh = kw["Tq"], kw["Tk1"] + kw.get("Tk2", 0), kw["dh"]
    masked, two, kvidx = "masks" in kw, kw.get("Tk2", 0) > 0, "ia" in kw
    if Tq <= 32 and Tk >= 128 and dh <= 64 and not masked and not two:
        return "stream1"
    if Tq > 128 and not masked and not two and not kvidx:
        return "stream3"
    if (Tq + 31) // 32 == 9:
        return "res9"
    if dh <= 64 and Tq <= 128 and Tk <= 64:
        return "res2"
    return "res4" if Tq <= 128 else "res8"
