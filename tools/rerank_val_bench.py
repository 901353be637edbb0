#!/usr/bin/env python3
"""Times of the two kernels of the two-stage validation at CIRR-val size (4181 queries x 2297 gallery images, top 200):
sprc_topk_wide at k = 200 and k = 64 against sprc_topk at k = 64 on the same score matrix, and sprc_rerank_order at 4181 x 200.
Timing pattern of tools/README.md: warm-up, HIP events around one launch, best and median of several.
Usage (GPU box): tools/rerank_val_bench.py [nq N]"""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sprc_amd import engine as E  # noqa: E402

NQ = int(sys.argv[1]) if len(sys.argv) > 1 else 4181
N = int(sys.argv[2]) if len(sys.argv) > 2 else 2297
DEV = "cuda:0"


def timed(fn, warm=3, reps=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) * 1e3)
    ms.sort()
    return {"best_us": round(ms[0], 1), "median_us": round(ms[len(ms) // 2], 1)}


def main():
    g = torch.Generator(device=DEV)
    g.manual_seed(0)
    sim = torch.rand((NQ, N), generator=g, device=DEV) * 1.1 - 0.2
    ref = torch.randint(0, N, (NQ,), generator=g, device=DEV, dtype=torch.int32)
    out = {"nq": NQ, "N": N, "device": torch.cuda.get_device_name(0), "row_read_MB": round(NQ * N * 4 / 1e6, 1)}
    out["sprc_topk k=64"] = timed(lambda: E.topk(sim, 64))
    out["sprc_topk_wide k=64"] = timed(lambda: E.topk_wide(sim, 64))
    out["sprc_topk_wide k=200 skip"] = timed(lambda: E.topk_wide(sim, 200, skip=ref))
    out["sprc_topk_wide k=256"] = timed(lambda: E.topk_wide(sim, 256))
    _, cand = E.topk_wide(sim, min(200, N - 1), skip=ref)
    prob = torch.rand(cand.shape, generator=g, device=DEV)
    listed = torch.randint(0, N, (NQ, 7), generator=g, device=DEV, dtype=torch.int32)
    rank = torch.randint(0, N, (NQ, 7), generator=g, device=DEV, dtype=torch.int32)
    out[f"sprc_rerank_order T={cand.shape[1]} L=7"] = timed(lambda: E.rerank_order(cand, prob, listed, rank))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
