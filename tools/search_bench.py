#!/usr/bin/env python3
"""Index search against its alternatives on one GPU, in one process, arms alternating inside every repetition (HIP events):

  (a) stream   E.search_topk: sprc_sim_max_stream + two-level top-k              (fp16 gallery)
  (a1) ..sim   its score kernel alone -> the achieved gallery bytes / s
  (b) gemm16   E.topk(E.sim_max(q16, g16), k): the 16-bit GEMM path + one-level top-k
  (b2) gemm16+2lvl  E.sim_max into a segmented buffer + E.topk_segmented (what Searcher runs above its nq threshold)
  (c) gemm32   fp32 sim_max + topk (the default rank_dtype); skipped when the fp32 gallery does not fit --fp32-budget-gb
  (d) copy     torch device-to-device copy of the fp16 gallery bytes (read + write): the box's streaming rate

    python tools/search_bench.py [--sizes 2297,123403,1000000] [--nq 1,8,32,64,256] [-k 50] [--reps 20] [--warmup 3] [--out FILE]

Synthetic unit-norm gallery and queries.  Per (N, nq): median [min .. max] microseconds per arm over the repetitions, the spread
of (a) and (b), and for (a1) / (d) the bytes / s.

    python tools/search_bench.py --query-split [--sizes 123403] [--reps 10]

Report only: one whole `Searcher` query on the full-depth synthetic ViT-g model (fp16 engine), split into reference embeddings (a stored
name: a lookup; an image file: decode + transform + ViT), fuse and rank, each phase ended by a device synchronisation.

    python tools/search_bench.py --filter [--sizes 123403,1000000] [--nq 1,32,64,256] [-k 50] [--reps 20] [--warmup 3] [--out FILE]

The filtered search against what there is without it, same protocol, for row lists of M = N (the identity list), N - 100, N / 3,
N / 100 and 1000 random ascending rows:

  (r) rows     E.search_topk(rows=): sprc_sim_max_stream_rows on the listed images + two-level top-k on M scores
  (r1) ..sim   its score kernel alone -> the achieved bytes / s of the listed images
  (p) plain    E.search_topk without a list: what any query costs without the filter (it cannot filter)
  (g) gather   feats.index_select(0, rows) + E.search_topk on the copy, the copy timed: the filter without the kernel
               (its indices are positions in the copy)
  (g+) ..map   the same with the positions mapped back to gallery rows: what a caller of (g) has to run to get what (r) returns
  (m) mask     above 32 queries only: E.sim_max (GEMM) on the whole gallery + -inf on the unlisted columns + E.topk_segmented

    python tools/search_bench.py --per-query [--sizes 123403,1000000] [--nq 1,8,32] [-k 50] [--reps 20] [--warmup 3] [--out FILE]

Per-query filters against what there is without them, same protocol: every query has its own random ascending list of N / 100 or
N / 3 rows, or the whole gallery minus 100 rows of its own; one more row gives every query the whole gallery (all-ones words: the
price of the bit test alone).  The union of the lists is what (q) and (u) walk.

  (q) admit    one E.search_topk(rows=union, admit=): sprc_sim_max_stream_admit + two-level top-k on the union's scores
  (s) serial   nq E.search_topk(rows=list_b) calls of one query each: per-query filters without the kernel
  (u) union    E.search_topk(rows=union) without admit: what the mask costs (it cannot filter per query)
  (q1) ..sim   the admit kernel alone -> the achieved bytes / s of the listed images"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from sprc_amd import engine as E  # noqa: E402


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _gallery(N, gen, dev, chunk=65536):
    g = torch.empty((N, 32, 256), dtype=torch.float16, device=dev)
    for s in range(0, N, chunk):
        n = min(chunk, N - s)
        g[s:s + n] = _unit(torch.randn((n, 32, 256), generator=gen, device=dev)).to(torch.float16)
    return g


def _time(arms, reps, warmup):
    """arms: {name: fn}; every repetition runs every arm once, in order -> {name: [ms, ...]}"""
    out = {n: [] for n in arms}
    for r in range(warmup + reps):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                out[name].append(a.elapsed_time(b))
    return out


def _fmt(ms):
    return f"{statistics.median(ms) * 1e3:9.1f} [{min(ms) * 1e3:8.1f} .. {max(ms) * 1e3:8.1f}]"


def _clock():
    try:
        import subprocess
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return " | ".join(l.strip() for l in r.splitlines() if "sclk" in l or "mclk" in l)[:300]
    except Exception as e:       # the reading is optional
        return f"(no clock reading: {e})"


def query_split(a, say):
    import tempfile
    import numpy as np
    from PIL import Image
    from sprc_amd import synth
    from sprc_amd.blip_validate import model_fingerprint
    from sprc_amd.index import save_index
    from sprc_amd.model import get_model_class
    from sprc_amd.search import Searcher
    dev = "cuda:0"
    model = get_model_class("blip2_cir_align_prompt").from_pretrained(model_type="pretrain", compute_dtype="fp16", device=dev)
    model.init_synthetic(seed=1)
    feats, raw = model.extract_target_features(synth.make_images(2, seed=3).to(dev))
    ids, mask, _ = synth.make_queries(1, 2, seed=4)
    gen = torch.Generator(device=dev).manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        save_index(f"{tmp}/s.safetensors", feats, ["a", "b"], raw=raw, checkpoint_sha256=model_fingerprint(model), raw_dtype=torch.float16,
                   feats_dtype=torch.float16)
        Image.fromarray(np.random.default_rng(0).integers(0, 256, size=(375, 500, 3), dtype=np.uint8)).save(f"{tmp}/q.png")
        s = Searcher(model, f"{tmp}/s.safetensors")
        for N in [int(x) for x in a.sizes.split(",")]:
            s.feats = _gallery(N, gen, dev)
            for what, ref in (("stored reference", ["a"]), ("image file (500 x 375 PNG)", [Path(f"{tmp}/q.png")])):
                rows = []
                for r in range(a.warmup + a.reps):
                    t = {}
                    s.search_ids(ref, ids, mask, a.k, timings=t)
                    if r >= a.warmup:
                        rows.append(t)
                med = {k: statistics.median(x[k] for x in rows) for k in rows[0]}
                say(f"query split, N = {N}, k = {a.k}, {what}: reference {med['reference_ms']:.3f} ms, fuse {med['fuse_ms']:.3f} ms, rank {med['rank_ms']:.3f} ms "
                    f"(medians of {a.reps}; host wall time per phase, device idle at each boundary)")


def _gather_search(q16, g16, rows64, rows, k):
    """arm (g) finished: the copy's positions mapped back to gallery rows, as (r) returns them"""
    v, i = E.search_topk(q16, g16.index_select(0, rows64), k)
    return v, torch.where(i < 0, i, rows[i.clamp(min=0)])


def filter_bench(a, say):
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    for N in [int(x) for x in a.sizes.split(",")]:
        g16 = _gallery(N, gen, dev)
        say(f"\nN = {N}  ({g16.numel() * 2 / 2**20:.0f} MiB fp16)")
        perm = torch.randperm(N, generator=gen, device=dev)
        lists = [("N (identity)", torch.arange(N, device=dev))] + [(what, perm[:m].sort().values) for what, m in
                 (("N - 100", N - 100), ("N / 3", N // 3), ("N / 100", N // 100), ("1000", min(1000, N)))]
        for nq in [int(x) for x in a.nq.split(",")]:
            q16 = _unit(torch.randn((nq, 256), generator=gen, device=dev)).to(torch.float16).contiguous()
            for what, rows64 in lists:
                rows = rows64.to(torch.int32).contiguous()
                M = rows.shape[0]
                sim_r = torch.empty((nq, M), dtype=torch.float32, device=dev)
                arms = {
                    "r": lambda: E.search_topk(q16, g16, a.k, rows=rows),
                    "p": lambda: E.search_topk(q16, g16, a.k),
                    "g": lambda: E.search_topk(q16, g16.index_select(0, rows64), a.k),
                    "g+": lambda: _gather_search(q16, g16, rows64, rows, a.k),
                    "r1": lambda: E.sim_max_stream(q16, g16, out=sim_r, rows=rows),
                }
                if nq > 32:
                    sim_m = E.segmented_sim_buffer(nq, N, dev)
                    off = torch.full((N,), float("-inf"), dtype=torch.float32, device=dev)
                    off[rows64] = 0.0
                    arms["m"] = lambda: E.topk_segmented(E.sim_max(q16, g16, out=sim_m).add_(off), a.k)
                t = _time(arms, a.reps, a.warmup)
                vr, ir = E.search_topk(q16, g16, a.k, rows=rows)
                vg, ig = _gather_search(q16, g16, rows64, rows, a.k)
                assert torch.equal(ir, ig) and ir.dtype == ig.dtype and torch.equal(vr, vg)
                med = {n: statistics.median(x) for n, x in t.items()}
                spread = {n: max(x) - min(x) for n, x in t.items()}
                seg, S = E.search_segments(nq, M)
                line = (f"  nq={nq:4d} M={M:8d} [{what:>12s}] S={S:3d}  (r) rows {_fmt(t['r'])}   (p) plain {_fmt(t['p'])}   (g) gather {_fmt(t['g'])}   (g+) gather+map {_fmt(t['g+'])}"
                        + (f"   (m) gemm+mask {_fmt(t['m'])}" if "m" in t else ""))
                say(line)
                say(f"           r/g = {med['r'] / med['g']:5.2f} (spread of the two {max(spread['r'], spread['g']) * 1e3:7.1f} us)   r/g+ = {med['r'] / med['g+']:5.2f} "
                    f"(spread {max(spread['r'], spread['g+']) * 1e3:7.1f} us)   r/p = {med['r'] / med['p']:5.2f} "
                    f"(spread {max(spread['r'], spread['p']) * 1e3:7.1f} us)"
                    + (f"   r/m = {med['r'] / med['m']:5.2f} (spread {max(spread['r'], spread['m']) * 1e3:7.1f} us)" if "m" in t else "")
                    + f"   (r1) rows kernel {_fmt(t['r1'])} = {M * 16384 * -(-nq // 32) / med['r1'] / 1e9:6.2f} TB/s of listed images")
                del sim_r
        del g16, perm, lists
        torch.cuda.empty_cache()


def _per_query_lists(N, nq, m, minus, gen, dev):
    """nq ascending int32 row lists: m random rows each, or (minus) all rows but m random ones; m = None: all rows."""
    out = []
    for _ in range(nq):
        if m is None:
            out.append(torch.arange(N, device=dev, dtype=torch.int32))
            continue
        perm = torch.randperm(N, generator=gen, device=dev)
        out.append((perm[m:] if minus else perm[:m]).sort().values.to(torch.int32).contiguous())
    return out


def per_query_bench(a, say):
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(0)
    for N in [int(x) for x in a.sizes.split(",")]:
        g16 = _gallery(N, gen, dev)
        say(f"\nN = {N}  ({g16.numel() * 2 / 2**20:.0f} MiB fp16)")
        for nq in [int(x) for x in a.nq.split(",")]:
            if not 1 <= nq <= 32:
                raise SystemExit("--per-query: one block of queries, nq in 1 .. 32")
            q16 = _unit(torch.randn((nq, 256), generator=gen, device=dev)).to(torch.float16).contiguous()
            for what, m, minus in (("N / 100 each", N // 100, False), ("N / 3 each", N // 3, False), ("N - 100 each", 100, True), ("N each (ones)", None, False)):
                lists = _per_query_lists(N, nq, m, minus, gen, dev)
                bits = torch.zeros(N, dtype=torch.int64, device=dev)
                for b, rows_b in enumerate(lists):
                    bits[rows_b.long()] |= 1 << b
                union64 = torch.nonzero(bits).flatten()
                union = union64.to(torch.int32).contiguous()
                w = bits[union64]
                admit = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32).view(1, -1).contiguous()
                M = union.shape[0]
                sim_q = torch.empty((nq, M), dtype=torch.float32, device=dev)
                qs = [q16[b:b + 1].contiguous() for b in range(nq)]
                arms = {
                    "q": lambda: E.search_topk(q16, g16, a.k, rows=union, admit=admit),
                    "s": lambda: [E.search_topk(qs[b], g16, a.k, rows=lists[b]) for b in range(nq)],
                    "u": lambda: E.search_topk(q16, g16, a.k, rows=union),
                    "q1": lambda: E.sim_max_stream(q16, g16, out=sim_q, rows=union, admit=admit),
                }
                t = _time(arms, a.reps, a.warmup)
                vq, iq = E.search_topk(q16, g16, a.k, rows=union, admit=admit)
                for b in range(nq):
                    vs, js = E.search_topk(qs[b], g16, a.k, rows=lists[b])
                    assert torch.equal(iq[b:b + 1], js) and torch.equal(vq[b:b + 1], vs)
                med = {n: statistics.median(x) for n, x in t.items()}
                spread = {n: max(x) - min(x) for n, x in t.items()}
                qs_spread, qu_spread = max(spread["q"], spread["s"]), max(spread["q"], spread["u"])
                ahead = med["s"] - med["q"]
                say(f"  nq={nq:3d} [{what:>13s}] union M={M:8d} S={E.search_segments(nq, M)[1]:3d}  (q) admit {_fmt(t['q'])}   (s) serial {_fmt(t['s'])}   (u) union {_fmt(t['u'])}")
                say(f"           s/q = {med['s'] / med['q']:6.2f}  ((q) ahead by {ahead * 1e3:9.1f} us; spread of the two arms {qs_spread * 1e3:7.1f} us: "
                    f"{'ahead' if ahead > qs_spread else 'behind' if -ahead > qs_spread else 'level'})   q/u = {med['q'] / med['u']:5.2f} (spread {qu_spread * 1e3:7.1f} us)"
                    f"   (q1) admit kernel {_fmt(t['q1'])} = {M * 16384 / med['q1'] / 1e9:6.2f} TB/s of listed images")
                del sim_q, bits, lists, union, union64, admit
        del g16
        torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--query-split", action="store_true")
    p.add_argument("--filter", action="store_true")
    p.add_argument("--per-query", action="store_true")
    p.add_argument("--sizes", default=None, help="default 2297,123403,1000000; --per-query: 123403,1000000")
    p.add_argument("--nq", default=None, help="default 1,8,32,64,256; --per-query: 1,8,32")
    p.add_argument("-k", type=int, default=50)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--fp32-budget-gb", type=float, default=40.0)
    p.add_argument("--out", default=None)
    a = p.parse_args(argv)
    a.sizes = a.sizes or ("123403,1000000" if a.per_query else "2297,123403,1000000")
    a.nq = a.nq or ("1,8,32" if a.per_query else "1,8,32,64,256")
    dev = "cuda:0"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"search_bench: k={a.k} reps={a.reps} warmup={a.warmup}  device={torch.cuda.get_device_name(0)}  times in us: median [min .. max]")
    say(f"clocks: {_clock()}")
    if a.query_split or a.filter or a.per_query:
        (query_split if a.query_split else filter_bench if a.filter else per_query_bench)(a, say)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lines) + "\n")
        return lines
    gen = torch.Generator(device=dev).manual_seed(0)
    for N in [int(x) for x in a.sizes.split(",")]:
        g16 = _gallery(N, gen, dev)
        gbytes = g16.numel() * 2
        with_c = gbytes * 2 <= a.fp32_budget_gb * 2**30
        g32 = g16.float() if with_c else None
        dst = torch.empty_like(g16)
        say(f"\nN = {N}  ({gbytes / 2**20:.0f} MiB fp16)" + ("" if with_c else "  [arm (c) skipped: the fp32 gallery exceeds --fp32-budget-gb]"))
        for nq in [int(x) for x in a.nq.split(",")]:
            q16 = _unit(torch.randn((nq, 256), generator=gen, device=dev)).to(torch.float16).contiguous()
            q32 = q16.float()
            sim_a = torch.empty((nq, N), dtype=torch.float32, device=dev)
            sim_b = torch.empty((nq, N), dtype=torch.float32, device=dev)
            sim_s = E.segmented_sim_buffer(nq, N, dev)
            arms = {
                "a": lambda: E.search_topk(q16, g16, a.k),
                "a1": lambda: E.sim_max_stream(q16, g16, out=sim_a),
                "b": lambda: E.topk(E.sim_max(q16, g16, out=sim_b), a.k),
                "b2": lambda: E.topk_segmented(E.sim_max(q16, g16, out=sim_s), a.k),
                "d": lambda: dst.copy_(g16),
            }
            if with_c:
                arms["c"] = lambda: E.topk(E.sim_max(q32, g32, out=sim_b), a.k)
            t = _time(arms, a.reps, a.warmup)
            va, ia = E.search_topk(q16, g16, a.k)
            vb, ib = E.topk(E.sim_max_stream(q16, g16), a.k)
            assert torch.equal(ia, ib) and torch.equal(va, vb)
            ma, mb = statistics.median(t["a"]), statistics.median(t["b"])
            spread = max(max(t["a"]) - min(t["a"]), max(t["b"]) - min(t["b"]))
            seg, S = E.search_segments(nq, N)
            say(f"  nq={nq:4d} S={S:3d}  (a) stream+2lvl {_fmt(t['a'])}   (b) gemm16+topk {_fmt(t['b'])}   (b2) gemm16+2lvl {_fmt(t['b2'])}"
                + (f"   (c) gemm32+topk {_fmt(t['c'])}" if with_c else ""))
            say(f"           b/a = {mb / ma:5.2f}  (a faster by {(mb - ma) * 1e3:8.1f} us; spread of the two arms {spread * 1e3:7.1f} us)"
                f"   (a1) stream kernel {_fmt(t['a1'])} = {gbytes / statistics.median(t['a1']) / 1e9:6.2f} TB/s gallery"
                f"   (d) copy {_fmt(t['d'])} = {gbytes / statistics.median(t['d']) / 1e9:6.2f} TB/s read (+ as much written)")
            del sim_a, sim_b, sim_s
        del g16, g32, dst
        torch.cuda.empty_cache()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
