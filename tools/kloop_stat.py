#!/usr/bin/env python3
"""Steady-state K loop of the 256 x 256 GEMM kernels in a `hipcc -S --cuda-device-only` listing: length, MFMAs, v_readfirstlane / waterfall loops
(a buffer descriptor that ended up in VGPRs: guide T20), v_readlane (spilled SGPRs), SALU / VALU counts; and the staging skeleton (loads, barriers,
counted waits) of the live and of the dead-wave steady loop, which have to agree.  A healthy loop: 217 / 218 / 214 instructions, 64 MFMAs,
0 waterfalls, 0 readlanes, 1 VALU (a v_cmp of the wave-group flag).
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -S --cuda-device-only -o x.s tools/kloop_probe.hip; python tools/kloop_stat.py x.s
(tests/test_kloop_listing.py runs exactly this on every CPU test pass: the regression it guards against is silent -- all parity tests stay green.)"""
import re
import sys

KERNELS = {"qkv-like (fp16 -> fp16)": "_ZN4sprc16gemm_anti_kernelIDF16_DF16_Li0ELb0ELb0ELb0EEEvNS_10GemmParamsE",
           "fc1-like (fp16 -> fp16, GELU)": "_ZN4sprc16gemm_anti_kernelIDF16_DF16_Li1ELb0ELb0ELb0EEEvNS_10GemmParamsE",
           "proj / fc2-like (fp16 -> fp32 + residual)": "_ZN4sprc16gemm_anti_kernelIDF16_fLi0ELb0ELb0ELb0EEEvNS_10GemmParamsE"}


def kernel_loops(lines, name):
    """-> (instruction lines of the kernel `name`, [(first, last)] of every back-edge loop in it, conditional or not), or None if it is not in the listing"""
    idx = [k for k, l in enumerate(lines) if l.startswith(name + ":")]
    if not idx:
        return None
    i = j = idx[0]
    while "s_endpgm" not in lines[j]:
        j += 1
    body = [l for l in lines[i:j] if l.strip() and not l.strip().startswith(";")]
    labels = {}
    for k, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = k
    loops = []
    for k, l in enumerate(body):
        m = re.search(r"s_c?branch\w* (\.LBB\d+_\d+)", l)       # hipcc may rotate a loop so that its only back edge is an unconditional s_branch
        if m and labels.get(m.group(1), k) < k:
            loops.append((labels[m.group(1)], k))
    return body, loops


def count(seg, prefix):
    return sum(x.strip().startswith(prefix) for x in seg)


def shortest_loop(body, loops, whole=False, **counts):
    """the shortest loop holding exactly these instruction counts (keyword = mnemonic prefix), as a list of stripped lines, or None.
    whole: up to the LAST back edge to its header that keeps the counts (a conditional wait in the latch: `s_cbranch header; s_waitcnt; s_branch header`)"""
    fit = [(k - a, a, k) for a, k in loops if all(count(body[a:k], p) == n for p, n in counts.items())]
    if not fit:
        return None
    a = min(fit)[1]
    k = (max if whole else min)(k for _, a2, k in fit if a2 == a)
    return [x.strip() for x in body[a:k]]


def steady_loop(lines, name):
    """-> dict of counts over the live steady loop of the kernel `name`: the shortest back-edge loop that holds exactly the 64 MFMAs of one K-tile
    pair (the run-time tail loop holds 32, the outer loops more).  None if the kernel is not in the listing."""
    kl = kernel_loops(lines, name)
    if kl is None:
        return None
    seg = shortest_loop(*kl, v_mfma=64)
    if seg is None:
        return {"kernel_lines": len(kl[0]), "len": 0, "mfma": 0, "waterfall": -1, "readfirstlane": -1, "readlane": -1, "salu": -1, "valu": -1}
    return {"kernel_lines": len(kl[0]), "len": len(seg), "mfma": count(seg, "v_mfma"), "readfirstlane": count(seg, "v_readfirstlane"),
            "waterfall": count(seg, "s_cbranch_execnz"), "readlane": count(seg, "v_readlane"),
            "salu": count(seg, "s_"), "valu": sum(x.startswith("v_") and "mfma" not in x for x in seg)}


def skeleton(seg):
    """the staging protocol of a loop body: L = LDS-DMA load, B = s_barrier, W3 / W4 = the counted waits the source writes.  (Other vmcnt values are
    hipcc's own: its LDS-DMA alias tracking puts vmcnt(13/12/10/8) before the first fragment read of a live loop.)"""
    tok = {"s_barrier": "B", "s_waitcnt vmcnt(3)": "W3", "s_waitcnt vmcnt(4)": "W4"}
    return ["L" if x.startswith("buffer_load") else tok[x] for x in seg if x.startswith("buffer_load") or x in tok]


def live_and_dead_skeletons(lines, name):
    """-> (skeleton of the live steady loop, skeleton of the dead-wave steady loop: the shortest loop with no MFMA, 8 barriers and 16 loads)"""
    body, loops = kernel_loops(lines, name)
    live, dead = shortest_loop(body, loops, True, v_mfma=64), shortest_loop(body, loops, True, v_mfma=0, s_barrier=8, buffer_load=16)
    return live and skeleton(live), dead and skeleton(dead)


def same_cycle(a, b):
    return a is not None and b is not None and len(a) == len(b) and any(b[i:] + b[:i] == a for i in range(max(len(b), 1)))


if __name__ == "__main__":
    for path in sys.argv[1:]:
        lines = open(path).read().split("\n")
        for what, name in KERNELS.items():
            print(path.split("/")[-1], what, steady_loop(lines, name))
            live, dead = live_and_dead_skeletons(lines, name)
            print("    live", " ".join(live or []), "\n    dead", " ".join(dead or []), "\n    same cycle:", same_cycle(live, dead))
