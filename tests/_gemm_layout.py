"""GEMM layout cases (tests/test_gemm_layout.py checks them on the host, tests/test_gemm_layout_gpu.py runs them): small products whose
operands, output, bias and residual live where the engine's real launches put them -- padded leading dimensions, offset pointers, row
maps with partial last groups, an output that aliases the residual -- inside poisoned buffers, so that a row offset formed with the wrong
leading dimension, a store past N, a map applied twice or a read of a pad column is an error of order 1, a NaN, or a changed guard byte.

Layout of every buffer (`Placed`): [guard >= G rows, a multiple of 256 bytes | element offset | P physical rows of ld elements | guard].
The base the device hands out is 256-byte aligned, so the pointer's alignment is exactly the element offset's.  Operand and residual
buffers are filled with NaN (0x7f bytes for e4m3fn and for split rows: NaN as fp16 and as e4m3), the output with a fixed NaN bit pattern
per type that is compared as integers.

Which kernel a forced SPRC_GEMM_TILE selects (read off launch() in sprc_amd/csrc/gemm_impl.hpp), by operand type:
    value   bf16 / fp16                        split-precision (k8 > 0)          fp8               fp32          max32 (16-bit | fp32)
    1       64x64: 4-stage ring `k64r` when    as bf16 / fp16                    128x128 `k128`    `k128`        `k128`
            the grid is <= 2 x CUs workgroups,
            else its 2-stage form `k64s`
    2       `k128`                             `k128`                            `k128`            `k128`        `k128`
    4       256x256 anti-phase `anti`          `anti`                            `anti`            `lock256`     `anti` | `lock256`
    14      lock-step 256x256 `lock256`        `k128` (no lock-step MIX kernel)  `lock256`         `lock256`     `lock256`
Automatic dispatch (0) adds the peeled split: `anti` on the first Mm rows, then the remainder rows on `k64r` or `k128`, or -- with caller
scratch and K >= 4096 -- on the 8-way split-K launch of the 128x128 kernel (ring of 4 stages) plus splitk_reduce_kernel: `peel:anti+splitk`.
`expected_route` restates that rule; the GPU test calls it with the live CU count."""
from __future__ import annotations

import json
import math
import os
import sys
from dataclasses import dataclass, replace
from typing import List, Optional, Tuple

import torch

from sprc_amd import _lib as L
from sprc_amd import engine as E

G_ROWS = 3                                             # guard rows above and below every 2-D buffer
ES_OP = {"bf16": 2, "f16": 2, "f32": 4, "fp8": 1, "mix": 2}
ES_OUT = {"f32": 4, "bf16": 2, "f16": 2, "fp8": 1, "x3": 2}      # x3: ldc counts fp16 units, a row's written part is 4 N bytes
OP_DT = {"bf16": L.SPRC_BF16, "f16": L.SPRC_F16, "f32": L.SPRC_F32, "fp8": L.SPRC_FP8, "mix": L.SPRC_F16}
OUT_DT = {"f32": L.SPRC_F32, "bf16": L.SPRC_BF16, "f16": L.SPRC_F16, "fp8": L.SPRC_FP8, "x3": L.SPRC_F16X3}
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "fp8": torch.float8_e4m3fn}
# (bit pattern, bytes per element): NaN poison of operand buffers, NaN sentinel of output buffers
POISON = {"bf16": (0x7FC0, 2), "f16": (0x7E00, 2), "f32": (0x7FC00000, 4), "fp8": (0x7F, 1), "mix": (0x7F, 1)}
SENTINEL = {"f32": (0x7FC5A5A5, 4), "bf16": (0x7FC5, 2), "f16": (0x7E55, 2), "fp8": (0x7F, 1), "x3": (0x7F, 1)}
TILES = (1, 2, 4, 14)
KERNELS = ("k64r", "k64s", "k128", "anti", "lock256")
KILLED = (124, 134, 137, 139)                          # child statuses that mean a time limit, an abort or a fault (and any negative one)


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


# ---- the dispatcher, restated (launch<> in gemm_impl.hpp) ---------------------------------------------------------------------------
def expected_route(M: int, N: int, K: int, ncu: int, *, op: str, out: str = "f32", resid: bool = False, max32: bool = False,
                   dual: bool = False, mapped: bool = False, ldc: Optional[int] = None, scratch_floats: int = 0, forced: int = 0) -> str:
    mix, es = op == "mix", ES_OP[op]
    keff = 2 * K if mix else K                         # k8 = 2 K: K + k8 / 2 sixteen-bit units
    mult = 2 if dual else 1
    cfg = forced
    if es <= 2:
        if cfg == 0:
            tn256, tn128 = cdiv(N, 256), cdiv(N, 128)
            f256 = 1.35 if (keff <= 1024 and out == "f32" and not max32 and resid) else 1.0
            cost256 = lambda m: f256 * ((mult * cdiv(m, 256) * tn256 + ncu - 1) // ncu)      # noqa: E731

            def cost128(m):
                t = mult * cdiv(m, 128) * tn128
                full, last = t // (2 * ncu), t % (2 * ncu)
                return 0.7 * full + (0.0 if last == 0 else 0.42 if last <= ncu else 0.7)
            cA, cB, cC, Mm = cost128(M), cost256(M), 1e30, 0
            if not max32 and not dual and M > 256 and not mapped:
                for j in range(13):
                    m = (M // 256 - j) * 256
                    if m <= 0 or m == M:
                        continue
                    c = cost256(m) + cost128(M - m) + 0.08
                    if c < cC - 1e-9:
                        cC, Mm = c, m
            rem = M - Mm
            if cC + 0.25 < min(cA, cB):
                ld = N if ldc is None else ldc
                if rem <= 128 and keff >= 4096 and N % 4 == 0 and ld % 4 == 0 and scratch_floats >= 8 * rem * N:
                    return "peel:anti+splitk"
                if es == 2 and not max32 and cdiv(rem, 128) * tn128 <= ncu:
                    return "peel:anti+k64r"
                return "peel:anti+k128"
            cfg = 4 if cB <= cA else 2
            if cfg == 2 and not max32 and es == 2 and mult * cdiv(M, 128) * tn128 <= ncu:
                cfg = 1
        if cfg in (4, 10):
            return "anti"
    elif cfg == 0:
        cfg = 4 if cdiv(M, 256) * cdiv(N, 256) >= 1024 else 2
    if not mix and cfg in (4, 10, 14):
        return "lock256"
    if es == 2 and not max32 and cfg == 1:
        return "k64r" if mult * cdiv(M, 64) * cdiv(N, 64) <= 2 * ncu else "k64s"
    return "k128"


def peel_rows(M: int, N: int, K: int, ncu: int, **kw) -> int:
    """Rows of the main (256x256) launch of a peeled split: the same search as expected_route's."""
    mix = kw.get("op") == "mix"
    keff = 2 * K if mix else K
    f256 = 1.35 if (keff <= 1024 and kw.get("out", "f32") == "f32" and kw.get("resid")) else 1.0
    tn256, tn128 = cdiv(N, 256), cdiv(N, 128)
    best, Mm = 1e30, 0
    for j in range(13):
        m = (M // 256 - j) * 256
        if m <= 0 or m == M:
            continue
        t = cdiv(M - m, 128) * tn128
        c128 = 0.7 * (t // (2 * ncu)) + (0.0 if t % (2 * ncu) == 0 else 0.42 if t % (2 * ncu) <= ncu else 0.7)
        c = f256 * ((cdiv(m, 256) * tn256 + ncu - 1) // ncu) + c128 + 0.08
        if c < best - 1e-9:
            best, Mm = c, m
    return Mm


# ---- a case ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                   # "gemm" | "pair" | "sim"
    op: str
    out: str
    M: int
    N: int                      # sim: N = 32 x images
    K: int
    act: int = L.ACT_NONE
    bias: bool = True
    bias_off: int = 0           # floats from the aligned base
    resid: Optional[str] = None           # None | "own" | "alias"
    ldr: int = 0
    r_off: int = 0
    ldc: int = 0                # elements of the output type (x3: fp16 units; sim: floats)
    c_off: int = 0
    a_pad: int = 0              # BYTES added to a row of A / W (multiples of 16)
    w_pad: int = 0
    amap: Optional[Tuple[int, int, Tuple[int, ...]]] = None        # (rows_per_group, group_stride, offset per product)
    cmap: Optional[Tuple[int, int, Tuple[int, ...]]] = None
    tile: int = 0               # forced SPRC_GEMM_TILE (0: automatic dispatch)
    kernel: str = ""            # the route the case is for (expected_route at 256 CUs; automatic cases: at the partition's 64)
    scratch: bool = False
    cause: str = "-"            # what the layout is meant to provoke (the class itself is computed: epi_class)
    seed: int = 0
    prod0: int = 0              # a paired case's product p as a launch of its own draws that product's operands

    @property
    def nprod(self) -> int:
        return 2 if self.kind == "pair" else 1

    @property
    def krow(self) -> int:      # elements of the operand type in a row of A / W
        return 2 * self.K if self.op == "mix" else self.K

    @property
    def row_bytes(self) -> int:
        return 4 * self.N if self.out == "x3" else (self.N // 32) * 4 if self.kind == "sim" else self.N * ES_OUT[self.out]

    def route_args(self):
        return dict(op=self.op, out=self.out, resid=self.resid is not None, max32=self.kind == "sim", dual=self.kind == "pair",
                    mapped=self.amap is not None or self.cmap is not None, ldc=self.ldc, forced=self.tile)


def phys_rows(mp, prod: int, M: int) -> torch.Tensor:
    m = torch.arange(M)
    if mp is None:
        return m
    rpg, stride, offs = mp
    return (m // rpg) * stride + (m % rpg) + offs[prod]


def epi_class(c: Case) -> str:
    """epi_vec_ok / wide_ok of gemm_impl.hpp from the case's layout (buffer bases are 256-byte aligned)."""
    if c.kind == "sim":
        return "max32"
    es = ES_OUT[c.out]
    c_addr = c.c_off * es
    b_addr = c.bias_off * 4 if c.bias else 0
    r_addr = 0 if c.resid is None else c_addr if c.resid == "alias" else c.r_off * 4
    ldr = c.ldc if c.resid == "alias" else c.ldr
    vec = (c.N % 4 == 0 and c.ldc % 4 == 0 and (c.resid is None or ldr % 4 == 0) and c_addr % (4 * es) == 0 and b_addr % 16 == 0
           and r_addr % 16 == 0)
    if not vec:
        return "scalar"
    if es < 4 and c.N % 8 == 0 and c.ldc % 8 == 0 and c_addr % 16 == 0:
        return "w8"
    return "w4"


def class_causes(c: Case) -> set:
    """Every condition that on its own keeps the case off the next wider store path."""
    if c.kind == "sim":
        return set()
    es, cls, out = ES_OUT[c.out], epi_class(c), set()
    c_addr = c.c_off * es
    ldr = c.ldc if c.resid == "alias" else c.ldr
    if cls == "scalar":
        out |= {"n"} if c.N % 4 else set()
        out |= {"ldc"} if c.ldc % 4 else set()
        out |= {"ldr"} if c.resid is not None and ldr % 4 else set()
        out |= {"calign"} if c_addr % (4 * es) else set()
        out |= {"bias"} if c.bias and (c.bias_off * 4) % 16 else set()
        out |= {"ralign"} if c.resid == "own" and (c.r_off * 4) % 16 else set()
    elif cls == "w4" and es < 4:
        out |= {"n"} if c.N % 8 else set()
        out |= {"ldc"} if c.ldc % 8 else set()
        out |= {"calign"} if c_addr % 16 else set()
    return out


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------
@dataclass
class Placed:
    buf: torch.Tensor           # flat uint8 (host)
    off: int                    # byte offset of element (physical row 0, column 0) = what the pointer adds to the base
    ld_b: int                   # row pitch in bytes
    P: int                      # physical rows

    def rows(self, buf: Optional[torch.Tensor] = None, ld_b: Optional[int] = None) -> torch.Tensor:
        """[P, pitch] byte view of the rows (of `buf`: this layout over another copy of the buffer)"""
        ld = self.ld_b if ld_b is None else ld_b
        return torch.as_strided(self.buf if buf is None else buf, (self.P, ld), (ld, 1), self.off)


def _fill(nbytes: int, pattern: Tuple[int, int]) -> torch.Tensor:
    bits, es = pattern
    dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[es]
    return torch.full((nbytes // es,), bits, dtype=dt).view(torch.uint8)


def make_placed(P: int, ld: int, es: int, elem_off: int, pattern: Tuple[int, int], other_ld: int = 0) -> Placed:
    """other_ld: the leading dimension of the buffer a broken kernel could confuse this one with (C and the residual, A and W).  The guards
    are wide enough that every row offset formed with it still lands inside the allocation: such a bug fails a check, it cannot fault."""
    ld_b = ld * es
    guard = cdiv(max(G_ROWS * ld_b, 256) + (P + 2 * G_ROWS) * max(0, other_ld - ld) * es, 256) * 256
    total = cdiv(guard + elem_off * es + P * ld_b + guard + 256, 256) * 256       # never ends at its allocation's end
    return Placed(_fill(total, pattern), guard + elem_off * es, ld_b, P)


def _bytes2d(t: torch.Tensor) -> torch.Tensor:
    t = t.contiguous()
    return t.view(torch.uint8).reshape(t.shape[0], -1)


def _rand(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def decode_operand(b: torch.Tensor, op: str, K: int, weight: bool, cols: Optional[int] = None) -> torch.Tensor:
    """operand row bytes -> the float64 values the product multiplies (split rows: the three segments side by side, scaled)"""
    b = b.contiguous()
    if op == "mix":
        hi = b[:, :2 * K].contiguous().view(torch.float16).double()
        s1 = b[:, 2 * K:3 * K].contiguous().view(torch.float8_e4m3fn).double()
        s2 = b[:, 3 * K:4 * K].contiguous().view(torch.float8_e4m3fn).double()
        # activations [hi | (x - hi) 2^12 | x], weights [W_hi | W 2^6 | (W - W_hi) 2^18]; the e4m3 products enter scaled by 2^-18
        return torch.cat([hi, s1 * 2.0 ** -6, s2 * 2.0 ** -18] if weight else [hi, s1 * 2.0 ** -12, s2], dim=1)
    return b.view(TORCH_DT[op]).double()


def activation(z: torch.Tensor, act: int) -> torch.Tensor:
    if act == L.ACT_GELU:
        return torch.nn.functional.gelu(z)
    if act == L.ACT_QUICKGELU:
        return z * torch.sigmoid(1.702 * z)
    return z


def w_scale_of(c: Case) -> float:
    """Operand scales of the existing test whose bound the case takes (see `bounds`)."""
    if c.op in ("bf16", "f32") and c.out == "f32" and (c.act != L.ACT_NONE or c.resid is not None):
        return 0.1                                     # test_gemm_epilogues
    return 0.05


@dataclass
class Data:
    """Everything a launch of a case needs, on the host: the placed buffers and the scalars."""
    A: Placed
    W: List[Placed]
    bias: List[Optional[Placed]]
    resid: Optional[Placed]         # None: no residual, or the aliased form (the residual then sits in C)
    C: Placed
    ws: Optional[torch.Tensor]      # fp8: per-output-channel weight scales (fp32, aligned)
    a_scale: float
    out_scale: float
    written: torch.Tensor           # bool mask over C.buf: the bytes the launch must write
    scratch_floats: int = 0


def contiguous_case(c: Case, p: int = 0) -> Case:
    """Product p of the case as a single launch with every operand contiguous, aligned and unmapped (what the other operator tests
    launch): the same logical problem -- build() draws the operands from (seed, product) alone."""
    return replace(c, name=f"{c.name}/flat{p}", kind="sim" if c.kind == "sim" else "gemm", prod0=c.prod0 + p, bias_off=0, ldr=c.N if c.resid == "own" else 0,
                   r_off=0, ldc=(2 * c.N if c.out == "x3" else c.N // 32 if c.kind == "sim" else c.N), c_off=0, a_pad=0, w_pad=0, amap=None, cmap=None)


def build(c: Case) -> Data:
    """Draw the logical operands from the case's seeds and place them."""
    es_a, es_c = ES_OP[c.op], ES_OUT[c.out]
    s = c.seed * 16
    a_rows = [phys_rows(c.amap, p, c.M) for p in range(c.nprod)]
    c_rows = [phys_rows(c.cmap, p, c.M) for p in range(c.nprod)]
    Pa = int(max(r.max() for r in a_rows)) + 3
    Pc = int(max(r.max() for r in c_rows)) + 3
    lda, ldw = c.krow + c.a_pad // es_a, c.krow + c.w_pad // es_a
    A = make_placed(Pa, lda, es_a, 0, POISON[c.op], other_ld=ldw)
    Ws, biases, a_scale, ws = [], [], 0.0, None
    for p in range(c.nprod):
        if c.kind == "sim":
            x = torch.nn.functional.normalize(_rand((c.M, c.K), s + 1), dim=-1)
            w = torch.nn.functional.normalize(_rand((c.N, c.K), s + 2), dim=-1)
        elif c.op == "mix":
            x, w = _rand((c.M, c.K), s + 1 + 7 * (p + c.prod0), 1.5), _rand((c.N, c.K), s + 2 + 7 * (p + c.prod0), 0.04)
        else:
            x, w = _rand((c.M, c.K), s + 1 + 7 * (p + c.prod0)), _rand((c.N, c.K), s + 2 + 7 * (p + c.prod0), w_scale_of(c))
        if c.op == "mix":
            xa, wa = E.split_rows(x), E.split_rows(w, weight=True)
        elif c.op == "fp8":
            a_scale = float(torch.tensor(float(x.abs().max()) / 448.0, dtype=torch.float32))
            xa = (x / a_scale).clamp(-448, 448).to(torch.float8_e4m3fn)
            wa, ws = E.quantize_fp8_rows(w)
        else:
            xa, wa = x.to(TORCH_DT[c.op]), w.to(TORCH_DT[c.op])
        A.rows()[a_rows[p], :c.krow * es_a] = _bytes2d(xa)
        W = make_placed(c.N, ldw, es_a, 0, POISON[c.op], other_ld=lda)
        W.rows()[:, :c.krow * es_a] = _bytes2d(wa)
        Ws.append(W)
        if c.bias:
            b = make_placed(1, c.N, 4, c.bias_off, POISON["f32"])
            b.rows()[0, :] = _bytes2d((_rand((1, c.N), s + 3 + 7 * (p + c.prod0)) + 0.01 * torch.arange(c.N)[None, :]).float())[0]
            biases.append(b)
        else:
            biases.append(None)
    C = make_placed(Pc, c.ldc, es_c, c.c_off, SENTINEL[c.out], other_ld=c.ldr if c.resid == "own" else 0)
    written = torch.zeros(C.buf.numel(), dtype=torch.bool)
    wv = C.rows(written)
    R = None
    for p in range(c.nprod):
        wv[c_rows[p], :c.row_bytes] = True
        if c.resid is not None:
            r = _bytes2d(_rand((c.M, c.N), s + 4 + 7 * (p + c.prod0)).float())
            if c.resid == "alias":
                C.rows()[c_rows[p], :c.N * 4] = r
            else:
                if R is None:
                    R = make_placed(Pc, c.ldr, 4, c.r_off, POISON["f32"], other_ld=c.ldc)
                R.rows()[c_rows[p], :c.N * 4] = r
    d = Data(A, Ws, biases, R, C, ws, a_scale, 1.0, written)
    if c.out == "fp8":                                 # as test_gemm_fp8_operands: the largest value lands on the largest e4m3
        peak = max(float(z.abs().max()) for z in reference(c, d, scaled=False))
        d.out_scale = float(torch.tensor(448.0 / max(peak, 1e-6), dtype=torch.float32))
    return d


def _operands(c: Case, d: Data, p: int):
    es_a = ES_OP[c.op]
    a = d.A.rows()[phys_rows(c.amap, p, c.M), :c.krow * es_a]
    w = d.W[p].rows()[:, :c.krow * es_a]
    a, w = decode_operand(a, c.op, c.K, False), decode_operand(w, c.op, c.K, True)
    if c.op == "fp8":
        a, w = a * d.a_scale, w * d.ws.double()[:, None]
    return a, w


def _read_f32(pl: Placed, rows: torch.Tensor, n: int, buf=None, ld_b=None) -> torch.Tensor:
    return pl.rows(buf, ld_b)[rows, :n * 4].contiguous().view(torch.float32).double()


def reference(c: Case, d: Data, scaled: bool = True, fault: Optional[str] = None) -> List[torch.Tensor]:
    """float64 result per product, from the bytes in the placed buffers (so a misplaced operand shows as a NaN here too).
    `fault`: the planted faults of the checker self-test that change what is READ ("resid_ldc", "a_pad")."""
    outs = []
    for p in range(c.nprod):
        a, w = _operands(c, d, p)
        z = a @ w.t()
        if fault == "a_pad":                           # one pad element of A's row 0 enters product (0, 0)
            pad = d.A.rows()[phys_rows(c.amap, p, c.M)[:1], c.krow * ES_OP[c.op]:c.krow * ES_OP[c.op] + ES_OP[c.op]]
            z[0, 0] += float(decode_operand(pad, "fp8" if c.op == "mix" else c.op, 1, False)[0, 0]) * float(w[0, 0])
        if c.kind == "sim":
            outs.append(z.view(c.M, c.N // 32, 32).max(-1).values)
            continue
        if c.bias:
            z = z + _read_f32(d.bias[p], torch.zeros(1, dtype=torch.long), c.N)
        z = activation(z, c.act)
        if c.resid is not None:
            crow = phys_rows(c.cmap, p, c.M)
            src = d.C if c.resid == "alias" else d.resid
            z = z + _read_f32(src, crow, c.N, ld_b=d.C.ld_b * 4 // ES_OUT[c.out] if fault == "resid_ldc" else None)
        if c.out == "fp8" and scaled:
            z = z * d.out_scale
        outs.append(z)
    return outs


def encode_out(z: torch.Tensor, out: str) -> torch.Tensor:
    """float64 result -> the bytes of a stored row"""
    z32 = z.float()
    if out == "x3":
        return _bytes2d(E.split_rows(z32))
    if out == "fp8":
        return _bytes2d(z32.clamp(-448, 448).to(torch.float8_e4m3fn))
    return _bytes2d(z32.to(TORCH_DT[out]))


def decode_out(b: torch.Tensor, c: Case):
    """stored row bytes -> (value as float64, the hi8 segment of a split row or None)"""
    b = b.contiguous()
    if c.out == "x3":
        hi, lo8, hi8 = E.split_decode(b.view(torch.float16), c.N)
        return hi.double() + lo8.double(), hi8.double()
    if c.kind == "sim":
        return b.view(torch.float32).double(), None
    return b.view(TORCH_DT[c.out]).double(), None


def written_rows(c: Case, d: Data, Cbuf: torch.Tensor) -> List[torch.Tensor]:
    return [d.C.rows(Cbuf)[phys_rows(c.cmap, p, c.M), :c.row_bytes].contiguous() for p in range(c.nprod)]


def emulate(c: Case, d: Data, fault: Optional[str] = None):
    """What a correct kernel leaves behind: the float64 reference, rounded, stored through the case's layout.  Returns (C bytes, residual
    bytes or None).  `fault` plants one of the mistakes the checker has to catch."""
    Cb = d.C.buf.clone()
    ref = reference(c, d, fault=fault if fault in ("resid_ldc", "a_pad") else None)
    view = d.C.rows(Cb)
    for p in range(c.nprod):
        rows = phys_rows(c.cmap, p, c.M).clone()
        enc = _bytes2d(ref[p].float()) if c.kind == "sim" else encode_out(ref[p], c.out)
        if fault == "row_unmapped":                    # the last row stored at m * ldc instead of its mapped row
            assert int(rows[-1]) != c.M - 1
            rows[-1] = c.M - 1
        if fault == "lo_at_hi8":                       # the lo segment of a split row stored at the hi8 offset
            assert c.out == "x3"
            lo = enc[:, 2 * c.N:3 * c.N].clone()
            enc[:, 2 * c.N:3 * c.N] = view[rows, 2 * c.N:3 * c.N]
            enc[:, 3 * c.N:] = lo
        view[rows, :c.row_bytes] = enc
    one = _bytes2d(torch.ones((1, 1)).to(torch.float32 if c.kind == "sim" else TORCH_DT.get(c.out, torch.float16)))[0]
    crow = phys_rows(c.cmap, 0, c.M)
    if fault == "pad_col":
        view[int(crow[0]), c.row_bytes:c.row_bytes + len(one)] = one
    if fault == "guard_row":
        Cb[d.C.off - d.C.ld_b:d.C.off - d.C.ld_b + len(one)] = one
    if fault == "between_rows":
        gap = sorted(set(range(int(crow.max()))) - set(crow.tolist()))
        view[gap[0], :len(one)] = one
    return Cb, (None if d.resid is None else d.resid.buf.clone())


# ---- the bounds: restated from the operator tests, nothing new ----------------------------------------------------------------------
def bounds(c: Case, ref_max: float):
    """(atol, rtol, round the reference to bf16 first).  A layout does not change the arithmetic, so every bound is the one an existing
    test asserts for the same operand / output types, operand scales (w_scale_of) and a reduction at least as long:
      bf16 -> f32   bias only: test_gemm_bf16;  with activation / residual: test_gemm_epilogues (tests/test_ops_gpu.py)
      bf16 -> bf16  bias or GELU: test_gemm_bf16 / test_gemm_bf16_256_tile_and_peel (against the bf16-rounded reference);
                    with QuickGELU / residual: test_gemm_bf16_random_shapes_through_the_dispatcher
      bf16 / fp8 -> f16   test_gemm_f16_delta_output (the fp32 result rounded once to fp16)
      f32           test_gemm_f32;  with activation / residual: test_gemm_epilogues
      fp16 -> f32   test_gemm_fp16;  with an activation: test_gemm_fp16_random_shapes_through_the_dispatcher (tests/test_fp16_gpu.py)
      fp16 -> f16   GELU alone: test_gemm_fp16;  otherwise the random-shapes test
      fp8 -> f32 / bf16   test_gemm_fp8_operands (tests/test_fp8_gpu.py); fp8 output: its one-e4m3-step rule (check_values)
      split rows    test_split_precision_gemm_shapes: {f32: 3e-6, f16: 2^-11, x3: 5e-5} x max |result| (+ 3e-5 with GELU)
      -> x3 from plain fp16 operands: the fp32 bound of the same epilogue plus that test's x3 storage term, 5e-5 x max |result|
      max over 32   test_sim_max (f32 2e-6, bf16 1e-5), test_gemm_fp16_splitk_rowmaps_pair_and_sim (fp16 2e-6)"""
    K, plain, gelu = c.K, c.act == L.ACT_NONE and c.resid is None, c.act == L.ACT_GELU
    if c.kind == "sim":
        return ({"f32": 2e-6, "bf16": 1e-5, "f16": 2e-6}[c.op], 0.0, False)
    if c.op == "mix":
        return ({"f32": 3e-6, "f16": 2.0 ** -11, "x3": 5e-5}[c.out] * ref_max + (3e-5 if gelu else 0.0), 0.0, False)
    if c.out == "f16" and c.op in ("bf16", "fp8"):
        return (2e-3 * math.sqrt(K / 64) + 2e-3, 1e-3, False)
    if c.op == "bf16":
        if c.out == "f32":
            return (2e-3 * math.sqrt(K / 64), 1e-4, False) if plain else (3e-3, 1e-4, False)
        return (2e-2, 1e-2, True) if (c.resid is None and c.act != L.ACT_QUICKGELU) else (4e-2, 1.6e-2, False)
    if c.op == "f32":
        return (5e-5 * math.sqrt(K / 32), 1e-5, False) if plain else (1e-4, 1e-4, False)
    if c.op == "fp8":
        return (2e-3 * math.sqrt(K / 64), 1e-4, False) if c.out == "f32" else (3e-2, 1e-2, True)
    f32b = (3e-4 * math.sqrt(K / 64), 1e-5) if c.act == L.ACT_NONE else (4e-4 * math.sqrt(K / 64) + 1e-4, 1e-5)      # fp16 operands
    if c.out == "f32":
        return (*f32b, False)
    if c.out == "x3":
        return (f32b[0] + 5e-5 * ref_max + (3e-5 if gelu else 0.0), f32b[1], False)
    return (2e-3, 1.5e-3, False) if (gelu and c.resid is None) else (4e-3, 2e-3, False)


def check_values(c: Case, got_bytes: torch.Tensor, ref: torch.Tensor, stats: Optional[dict] = None) -> List[str]:
    """checks 1 and 3 on one product: finite at every written position, and within the bound of the float64 reference"""
    got, hi8 = decode_out(got_bytes, c)
    bad = []
    if not bool(torch.isfinite(got).all()):
        n = int((~torch.isfinite(got)).sum())
        return [f"poison: {n} of {got.numel()} written positions are not finite (first at {tuple((~torch.isfinite(got)).nonzero()[0].tolist())})"]
    if c.out == "fp8":                                 # test_gemm_fp8_operands: one e4m3 step (two subnormal steps near zero), few differ at all
        want = ref.float().clamp(-448, 448).to(torch.float8_e4m3fn).double()
        diff = (got - want).abs()
        ulp = (want.abs() * 2.0 ** -3).clamp_min(2.0 ** -8)
        if stats is not None:
            stats["fp8_n"] = stats.get("fp8_n", 0) + got.numel()
            stats["fp8_diff"] = stats.get("fp8_diff", 0) + int((diff > 0).sum())
        if bool((diff > ulp).any()):
            bad.append(f"float64: {int((diff > ulp).sum())} fp8 outputs more than one e4m3 step off (max {float(diff.max()):.3g})")
        elif got.numel() >= 4096 and float((diff > 0).float().mean()) >= 0.02:
            bad.append(f"float64: {float((diff > 0).float().mean()):.3%} of the fp8 outputs differ from the rounded reference")
        return bad
    atol, rtol, round_bf16 = bounds(c, float(ref.abs().max()))
    want = ref.float().to(torch.bfloat16).double() if round_bf16 else ref
    err = (got - want).abs()
    over = err > atol + rtol * want.abs()
    if bool(over.any()):
        i = tuple(over.nonzero()[0].tolist())
        bad.append(f"float64: {int(over.sum())} of {got.numel()} outputs outside atol {atol:.3g} rtol {rtol:.3g}; max error {float(err.max()):.3g}, "
                   f"first at {i}: got {float(got[i]):.6g} want {float(want[i]):.6g}")
    if hi8 is not None:                                # test_split_precision_gemm_chain: the hi8 segment holds the value to 4 bits
        lim = float(ref.abs().max()) * 2.0 ** -4 + 1e-4
        if not bool(((hi8 - ref).abs() <= lim).all()):
            bad.append(f"float64: hi8 segment off by {float(torch.nan_to_num((hi8 - ref).abs(), nan=float('inf')).max()):.3g} (> {lim:.3g})")
    return bad


def check(c: Case, d: Data, Cbuf: torch.Tensor, Rbuf: Optional[torch.Tensor], stats: Optional[dict] = None) -> List[str]:
    """Checks 1-3 of a launch's output buffers.  Returns one line per failed check (empty: passed)."""
    bad = []
    keep = ~d.written
    if not torch.equal(Cbuf[keep], d.C.buf[keep]):
        idx = ((Cbuf != d.C.buf) & keep).nonzero()[:, 0]
        rel = int(idx[0]) - d.C.off
        bad.append(f"guard: {idx.numel()} bytes of C outside the written set changed; first at byte {rel} from C = physical row "
                   f"{rel // d.C.ld_b}, byte {rel % d.C.ld_b} of the row (row width {c.row_bytes}, pitch {d.C.ld_b})")
    if d.resid is not None and Rbuf is not None and not torch.equal(Rbuf, d.resid.buf):
        bad.append(f"guard: {int((Rbuf != d.resid.buf).sum())} bytes of the residual buffer changed")
    got, ref = written_rows(c, d, Cbuf), reference(c, d)
    for p in range(c.nprod):
        if not bool(torch.isfinite(ref[p]).all()):
            bad.append("case: the float64 reference itself is not finite (placement mistake in the test)")
            continue
        bad += [f"product {p}: {m}" if c.nprod > 1 else m for m in check_values(c, got[p], ref[p], stats)]
    return bad


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# (op, out, activations built, residual allowed, paired launch allowed): dispatch / dispatch_mix of gemm_impl.hpp, gemm_impl() of gemm.hip
COMBOS = [("bf16", "f32", (0, 1, 2), True, True), ("bf16", "bf16", (0, 1, 2), True, True), ("bf16", "f16", (0,), False, True),
          ("f16", "f32", (0, 1, 2), True, True), ("f16", "f16", (0, 1, 2), True, True), ("f16", "x3", (0, 1), False, True),
          ("f32", "f32", (0, 1, 2), True, True),
          ("fp8", "f32", (0,), True, False), ("fp8", "bf16", (0,), True, False), ("fp8", "f16", (0,), False, False),
          ("fp8", "fp8", (0, 1, 2), True, False),
          ("mix", "f32", (0, 1), True, True), ("mix", "f16", (0, 1), True, True), ("mix", "x3", (0, 1), False, True)]
# (cause, N, ldc - row width, c_off, bias_off, residual, ldr - N, r_off); the row width is N (2 N fp16 units for split rows)
NARROW = [("-", 264, 8, 0, 0, "own", 4, 0), ("-", 8, 16, 0, 0, "own", 12, 4),
          ("n", 36, 4, 0, 0, "own", 8, 0), ("n", 516, 12, 0, 0, "own", 4, 0), ("n", 4, 4, 0, 0, "own", 8, 0), ("n", 12, 12, 0, 0, "own", 4, 4),
          ("ldc", 264, 4, 0, 0, "own", 8, 0), ("calign", 8, 8, 4, 0, "own", 4, 0),
          ("n", 130, 6, 0, 0, "own", 2, 0), ("ldc", 264, 2, 0, 0, "own", 4, 0), ("ldr", 264, 8, 0, 0, "own", 6, 0),
          ("calign", 36, 4, 1, 0, "own", 8, 0), ("calign", 516, 12, 2, 0, "own", 4, 0), ("bias", 264, 8, 0, 1, "own", 4, 0),
          ("ralign", 8, 8, 0, 0, "own", 4, 1)]
WIDE = [("-", 264, 8, 0, 0, "own", 4, 0), ("-", 4, 4, 0, 0, "own", 8, 4), ("-", 12, 4, 0, 0, "alias", 0, 0), ("-", 516, 4, 4, 0, "own", 8, 0),
        ("-", 8, 4, 0, 0, "alias", 0, 0), ("-", 36, 8, 4, 0, "alias", 0, 0),
        ("n", 130, 6, 0, 0, "own", 2, 0), ("n", 130, 2, 0, 0, "alias", 0, 0), ("ldc", 264, 2, 0, 0, "own", 6, 0), ("ldr", 264, 8, 0, 0, "own", 6, 0),
        ("calign", 36, 4, 1, 0, "own", 8, 0), ("calign", 516, 12, 2, 0, "alias", 0, 0), ("bias", 264, 8, 0, 1, "own", 4, 0),
        ("ralign", 8, 8, 0, 0, "own", 4, 1)]
SPLIT = [s for s in NARROW if s[1] % 4 == 0 and s[0] not in ("ldr", "ralign")]
M_SET = (1, 63, 65, 129, 257, 300)
# row maps: rows_per_group in {1, 32, 64}, stride > rows per group, offsets != 0; M_SET leaves every last group partial and the 32- and
# 1-row groups put group boundaries inside every tile
MAPS = [(None, None), ((32, 40, (3,)), None), (None, (64, 70, (5,))), ((1, 3, (2,)), (32, 48, (7,))), ((64, 80, (9,)), (1, 2, (1,)))]
PAIR_MAPS = ((32, 72, (2, 37)), (32, 72, (3, 38)))          # the paired launch's two offsets: rows [3, 35) and [38, 70) of every 72


def _k_of(op: str, i: int) -> int:
    return {"bf16": (128, 192)[i % 2], "f16": (192, 128)[i % 2], "f32": 96, "fp8": 256, "mix": 256}[op]


def _mk(name, kind, op, out, M, N, K, tile, i, *, act=0, bias=True, spec=None, maps=(None, None), **kw) -> Case:
    cause, _, dldc, c_off, bias_off, resid, dldr, r_off = spec
    width = 2 * N if out == "x3" else N
    pads = ((16, 48), (48, 16), (80, 32), (32, 112))[i % 4]                     # bytes; 48, 80 and 112 are no power of two
    c = Case(name=name, kind=kind, op=op, out=out, M=M, N=N, K=K, act=act, bias=bias, bias_off=bias_off if bias else 0, resid=resid,
             ldr=(N + dldr) if resid == "own" else 0, r_off=r_off if resid == "own" else 0, ldc=width + dldc, c_off=c_off,
             a_pad=pads[0], w_pad=pads[1], amap=maps[0], cmap=maps[1], tile=tile, cause=cause, seed=1000 * tile + i, **kw)
    return replace(c, kernel=expected_route(c.M, c.N, c.K, 256, **c.route_args()))


def forced_cases(tile: int) -> List[Case]:
    """The table one child process runs under SPRC_GEMM_TILE=tile."""
    cases, i = [], 0
    for op, out, acts, resid_ok, pair_ok in COMBOS:
        specs = WIDE if out == "f32" else SPLIT if out == "x3" else NARROW
        for spec in specs:
            cause, N = spec[0], spec[1]
            if not resid_ok:
                if cause in ("ldr", "ralign"):
                    continue
                spec = spec[:5] + (None, 0, 0)
            for bias, res in ((True, True), (True, False), (False, True), (False, False)):
                if (cause == "bias" and not bias) or (cause in ("ldr", "ralign") and not res) or (res and spec[5] is None):
                    continue
                sp = spec if res else spec[:5] + (None, 0, 0)
                feat = i % 6
                pair = feat == 5 and pair_ok
                maps = PAIR_MAPS if pair else MAPS[feat % 5]
                M = M_SET[i % 6] if not pair else M_SET[(i // 6) % 6]
                cases.append(_mk(f"t{tile}-{op}-{out}-{i}", "pair" if pair else "gemm", op, out, M, N, _k_of(op, i), tile, i,
                                 act=acts[(i // 2) % len(acts)], bias=bias, spec=sp, maps=maps))
                i += 1
    # the max over 32: ragged nq, ld_sim > images
    for op in ("bf16", "f16", "f32"):
        for nq, imgs in ((5, 7), (65, 9), (129, 3)):
            c = Case(name=f"t{tile}-sim-{op}-{nq}x{imgs}", kind="sim", op=op, out="f32", M=nq, N=32 * imgs, K=96 if op == "f32" else 128, bias=False,
                     ldc=imgs + 3, tile=tile, seed=1000 * tile + 900 + i)
            cases.append(replace(c, kernel=expected_route(c.M, c.N, c.K, 256, **c.route_args())))
            i += 1
    if tile == 1:
        # the 2-stage form of the 64x64 tile needs more than 2 x CUs workgroups: 24 x 24 tiles.  One case per reachable class and output type.
        wide = [("-", 1496, 8, 0, 0, "own", 4, 0), ("-", 1500, 4, 0, 0, "alias", 0, 0), ("n", 1498, 6, 0, 0, "own", 2, 0), ("ldr", 1496, 8, 0, 0, "own", 6, 0)]
        narrow = [("-", 1496, 8, 0, 0, "own", 4, 0), ("n", 1500, 4, 0, 0, "own", 8, 0), ("calign", 1496, 8, 4, 0, "own", 4, 0),
                  ("n", 1498, 6, 0, 0, "own", 2, 0), ("bias", 1496, 8, 0, 1, "own", 4, 0)]
        split = [("-", 1496, 8, 0, 0, None, 0, 0), ("n", 1500, 8, 0, 0, None, 0, 0), ("ldc", 1496, 2, 0, 0, None, 0, 0), ("calign", 1500, 8, 1, 0, None, 0, 0)]
        for op, out, specs in (("bf16", "f32", wide), ("bf16", "bf16", narrow), ("f16", "f16", narrow), ("f16", "x3", split), ("mix", "f32", wide[1:3])):
            for sp in specs:
                cases.append(_mk(f"t1-big-{op}-{out}-{i}", "gemm", op, out, 1500, sp[1], 256 if op == "mix" else 128, 1, i,
                                 act=(0, 1)[i % 2], bias=sp[0] == "bias" or i % 3 != 0, spec=sp, maps=MAPS[i % 5]))
                i += 1
    return cases


# automatic dispatch on a 64-CU partition stream (a quarter of a 256-CU MI355X): the peeled split and its three remainders.  (The cost model
# never leaves a 16-bit remainder on 128x128: one that fits a round of 64x64 tiles takes the ring, and a larger one costs 0.7 + 0.08 + 0.25 =
# 1.03 rounds against the one round that 256x256 on everything adds.  fp8 operands have no 64x64 tile, so theirs is the 128x128 remainder.)
def auto_cases() -> List[Case]:
    out = []
    for name, op, o, M, N, K, scratch, resid, route in (
            ("auto-splitk-bf16", "bf16", "f32", 1124, 4096, 4096, True, "own", "peel:anti+splitk"),
            ("auto-splitk-f16-f16", "f16", "f16", 1124, 4096, 4096, True, "own", "peel:anti+splitk"),
            ("auto-ring-bf16", "bf16", "f32", 1124, 4096, 2048, False, "own", "peel:anti+k64r"),
            ("auto-k128-fp8", "fp8", "bf16", 1124, 4096, 256, False, "own", "peel:anti+k128"),
            ("auto-ring-alias-f16", "f16", "f32", 1124, 4096, 2048, False, "alias", "peel:anti+k64r")):
        out.append(Case(name=name, kind="gemm", op=op, out=o, M=M, N=N, K=K, act=L.ACT_GELU if o == "f16" else L.ACT_NONE, bias=True,
                        resid=resid, ldr=N + 12 if resid == "own" else 0, r_off=4 if resid == "own" else 0, ldc=N + 8, c_off=0,
                        a_pad=48, w_pad=80, tile=0, kernel=route, scratch=scratch, seed=7000 + len(out)))
    return out


AUTO_NCU = 64


# ---- running a case on the GPU ----------------------------------------------------------------------------------------------------------
class Runner:
    def __init__(self, device: str = "cuda:0"):
        self.lib, self.dev = L.load(), device

    def _up(self, pl: Optional[Placed]):
        if pl is None:
            return None, None
        t = pl.buf.to(self.dev)
        assert t.data_ptr() % 256 == 0
        return t, t.data_ptr() + pl.off

    def run(self, c: Case, d: Data, stream: Optional[int] = None):
        """One launch of the case on freshly uploaded buffers.  Returns (C bytes, residual bytes or None, scratch tail intact)."""
        import ctypes as Ct
        keep = []
        tA, pA = self._up(d.A)
        tC, pC = self._up(d.C)
        tR, pR = self._up(d.resid)
        keep += [tA, tC, tR]
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        es_a = ES_OP[c.op]
        tS = None
        if c.kind == "sim":
            tW, pW = self._up(d.W[0])
            assert d.A.ld_b == c.K * es_a and d.W[0].ld_b == c.K * es_a
            L.check(self.lib.sprc_sim_max(pA, pW, pC, c.ldc, c.M, c.N // 32, c.K, OP_DT[c.op], st), "sprc_sim_max")
        else:
            gs = []
            tws = None if d.ws is None else d.ws.to(self.dev)
            if d.scratch_floats:
                tS = torch.full((d.scratch_floats + 64,), float("nan"), device=self.dev)
                tS.view(torch.int32)[d.scratch_floats:] = SENTINEL["f32"][0]
            for p in range(c.nprod):
                tW, pW = self._up(d.W[p])
                tB, pB = self._up(d.bias[p])
                keep += [tW, tB]
                g = L.GemmArgs()
                g.M, g.N, g.K, g.dtype, g.out_dtype, g.act, g.max32 = c.M, c.N, c.K, OP_DT[c.op], OUT_DT[c.out], c.act, 0
                g.k8 = 2 * c.K if c.op == "mix" else 0
                g.A, g.lda, g.W, g.ldw = pA, d.A.ld_b // es_a, pW, d.W[p].ld_b // es_a
                g.amap = E.rowmap(*((c.amap[0], c.amap[1], c.amap[2][p]) if c.amap else ()))
                g.cmap = E.rowmap(*((c.cmap[0], c.cmap[1], c.cmap[2][p]) if c.cmap else ()))
                g.bias = pB
                if c.resid is not None:
                    g.resid, g.ldr = (pC, c.ldc) if c.resid == "alias" else (pR, c.ldr)
                g.C, g.ldc = pC, c.ldc
                if tS is not None:
                    g.scratch, g.scratch_bytes = tS.data_ptr(), d.scratch_floats * 4
                if tws is not None:
                    assert tws.data_ptr() % 16 == 0
                    g.w_scale, g.a_scale = tws.data_ptr(), d.a_scale
                g.out_scale = d.out_scale if c.out == "fp8" else 0.0
                gs.append(g)
            if c.nprod == 2:
                L.check(self.lib.sprc_gemm_pair(Ct.byref(gs[0]), Ct.byref(gs[1]), st), "sprc_gemm_pair")
            else:
                L.check(self.lib.sprc_gemm(Ct.byref(gs[0]), st), "sprc_gemm")
        torch.cuda.synchronize()
        tail_ok = True if tS is None else bool((tS.view(torch.int32)[d.scratch_floats:] == SENTINEL["f32"][0]).all())
        return tC.cpu(), (None if tR is None else tR.cpu()), tail_ok


def run_checks(r: Runner, c: Case, stats: dict, stream: Optional[int] = None) -> List[str]:
    """Checks 1-5 of one case.  Returns the failures as 'check: detail' lines."""
    d = build(c)
    if c.scratch:
        rem = c.M - peel_rows(c.M, c.N, c.K, AUTO_NCU, op=c.op, out=c.out, resid=c.resid is not None)
        d.scratch_floats = 8 * rem * c.N
    Cb, Rb, tail = r.run(c, d, stream)
    bad = check(c, d, Cb, Rb, stats)
    if not tail:
        bad.append("guard: the sentinel behind the split-K scratch changed")
    Cb2, _, _ = r.run(c, d, stream)
    if not torch.equal(Cb, Cb2):
        bad.append(f"repeat: {int((Cb != Cb2).sum())} bytes differ between two launches")
    # check 4: the contiguous launch of the same logical problem
    got = written_rows(c, d, Cb)
    for p in range(c.nprod):
        tc = contiguous_case(c, p)
        dt = build(tc)
        dt.scratch_floats, dt.out_scale = d.scratch_floats, d.out_scale
        Ct_, _, _ = r.run(tc, dt, stream)
        flat = written_rows(tc, dt, Ct_)[0]
        same = torch.equal(flat, got[p])
        ca, cb = epi_class(c), epi_class(tc)
        if (ca == "scalar") != (cb == "scalar"):       # scalar against vector: counted for the summary line (test_gemm_layout_gpu.py)
            stats["mixed_pairs"] = stats.get("mixed_pairs", 0) + 1
            stats["mixed_equal"] = stats.get("mixed_equal", 0) + int(same)
        if not same:
            bad.append(f"invariance: product {p} differs from the contiguous launch in {int((flat != got[p]).sum())} bytes ({ca} against {cb})")
    return bad


def child_main(tile: int) -> None:
    """Body of the child process of one forced tile: one JSON line per failed check, a summary line last, exit status 0."""
    assert int(os.environ.get("SPRC_GEMM_TILE", "0")) == tile
    r = Runner()
    ncu = r.lib.sprc_stream_cus(None)
    stats, ran, skipped = {}, 0, 0
    for c in forced_cases(tile):
        route = expected_route(c.M, c.N, c.K, ncu, **c.route_args())
        if route != c.kernel:
            print(json.dumps({"skip": c.name, "wanted": c.kernel, "route": route, "ncu": ncu}), flush=True)
            skipped += 1
            continue
        try:
            bad = run_checks(r, c, stats)
        except L.SprcError as e:
            bad = [f"launch: {e}"]
        for m in bad:
            print(json.dumps({"case": c.name, "kernel": c.kernel, "class": epi_class(c), "cause": c.cause, "fail": m}), flush=True)
        ran += 1
    print(json.dumps({"done": True, "tile": tile, "ran": ran, "skipped": skipped, "ncu": ncu, **stats}), flush=True)


if __name__ == "__main__":
    child_main(int(sys.argv[1]))
