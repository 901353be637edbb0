"""Build libsprc_hip.so (gfx950) in-tree with hipcc.  `python -m sprc_amd.build [--force]`."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB = Path(__file__).resolve().parent / "libsprc_hip.so"
SOURCES = ["gemm.hip", "gemm_f16.hip", "gemm_f16e.hip", "gemm_fp8.hip", "gemm_f32.hip", "core.hip", "attention.hip", "rowops.hip", "rank.hip", "search.hip", "models.hip", "preprocess.hip", "train.hip", "optim.hip"]
# -fno-slp-vectorize: hipcc packs adjacent scalar fp32 ops into v_pk_fma_f32 / v_pk_mul_f32, which run SLOWER than the scalar
# pairs on gfx950 (measured on the GEMM GELU epilogue: 117 us packed vs ~45 us scalar per ViT fc1 launch)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-fno-slp-vectorize"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (Path(c).exists() or c == "hipcc"):
            return c
    raise RuntimeError("hipcc not found")


def _stale(out: Path, deps) -> bool:
    return (not out.exists()) or any(Path(d).stat().st_mtime > out.stat().st_mtime for d in deps)


def build(force: bool = False, verbose: bool = True, always: tuple = ()) -> Path:
    """force: recompile everything; always: sources recompiled even when their objects are up to date (the driver's build
    check names one small translation unit there, so that hipcc really runs wherever build() is called)."""
    hipcc = _hipcc()
    objdir = CSRC / "build"
    objdir.mkdir(exist_ok=True)
    headers = [CSRC / "common.hpp", CSRC / "gemm_impl.hpp", CSRC.parent.parent / "include" / "sprc.h"]

    def compile_one(src: str):
        obj = objdir / (src + ".o")
        if force or src in always or _stale(obj, [CSRC / src, *headers]):
            cmd = [hipcc, *FLAGS, "-c", str(CSRC / src), "-o", str(obj)]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(12, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    # (build.py itself is a dependency: the source LIST lives here -- a new translation unit must relink)
    if force or _stale(LIB, [*objs, Path(__file__)]):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(LIB), *map(str, objs)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
