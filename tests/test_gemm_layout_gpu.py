"""GEMM memory layouts on the GPU: every tile kernel and every epilogue store path on padded strides, offset pointers, row maps with
partial groups and an output that aliases the residual, inside poisoned buffers with guard bands (tests/_gemm_layout.py builds the cases,
tests/test_gemm_layout.py checks the table and the checker on the host).

Per case: (1) the float64 reference of the same rounded operands within the bound the operator tests already assert for that operand /
output pair (_gemm_layout.bounds lists where each comes from); (2) every byte of the output buffer outside the written set, and the whole
residual buffer, bit-identical to what was uploaded; (3) finite at every written position: no pad column, guard row or unmapped row of
A / W entered a product; (4) bit-identical to the contiguous, aligned, unmapped launch of the same logical problem on the same tile
kernel, whatever store path either takes; (5) two launches bit-identical.

Check 4, as measured on an MI355X (256 CUs).  The store paths did NOT agree at first: with an activation AND a residual, hipcc fused the
activation's last multiply with the residual add in some instantiations of epi_value and not in others -- 42 to 45 of the 232 to 237
scalar-against-vector pairs of every tile value differed in a last bit (every other pair was equal), and so did the 8- and the 4-column
path of one kernel on the fp16-output paired cases (1 or 2 bytes of 129 x 264 outputs).  epi_value now pins the activation's result
(an empty asm, no instruction); since then all 933 scalar-against-vector pairs and every vector pair are bit-identical, and bit equality
is asserted for every pair.  No launch of the engine combines an activation with a residual, so its results did not move.

The library reads SPRC_GEMM_TILE once per process, so each forced tile runs its whole table in a child process of its own."""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

import _gemm_layout as G  # noqa: E402
from sprc_amd import _lib as L  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
DEV = "cuda:0"
_DEAD = {"why": None}           # set when a child was killed, aborted or faulted: nothing more is started on the GPU from this module


def _alive():
    if _DEAD["why"]:
        pytest.fail(f"not started: {_DEAD['why']}")


@pytest.mark.parametrize("tile", G.TILES)
def test_layout_cases_under_a_forced_tile(tile):
    _alive()
    code = f"import sys; sys.path.insert(0, {str(ROOT / 'tests')!r}); import _gemm_layout as G; G.child_main({tile})"
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SPRC_GEMM_TILE=str(tile)),
                         capture_output=True, text=True)
    if run.returncode in G.KILLED or run.returncode < 0:
        _DEAD["why"] = f"the child of SPRC_GEMM_TILE={tile} ended with status {run.returncode}"
        pytest.fail(_DEAD["why"] + "\n" + run.stdout[-3000:] + run.stderr[-3000:])
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-4000:]
    lines = [json.loads(x) for x in run.stdout.splitlines() if x.startswith("{")]
    done = [x for x in lines if x.get("done")]
    assert len(done) == 1, run.stdout[-3000:]
    print(f"\n[gemm layout, SPRC_GEMM_TILE={tile}] {json.dumps(done[0])}")
    fails, skips = [x for x in lines if "fail" in x], [x for x in lines if "skip" in x]
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(json.dumps(x) for x in fails[:40])
    assert not skips and done[0]["skipped"] == 0, f"cases skipped at {done[0]['ncu']} CUs:\n" + "\n".join(json.dumps(x) for x in skips[:20])
    assert done[0]["ran"] == len(G.forced_cases(tile))
    if done[0].get("fp8_n"):       # test_gemm_fp8_operands: fewer than 2 % of the fp8 outputs differ from the rounded reference at all
        assert done[0]["fp8_diff"] < 0.02 * done[0]["fp8_n"]


@pytest.fixture(scope="module")
def partition():
    """A CU-masked stream over a quarter of the chip (tests/test_ops_gpu.py::test_cu_partition_streams): the dispatcher's cost model then
    peels at shapes a quarter the size."""
    _alive()
    assert "SPRC_GEMM_TILE" not in os.environ, "the automatic cases need the automatic dispatcher"
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.sprc_stream_create_partition(0, 4, C.byref(h)), "sprc_stream_create_partition")
    yield h.value, lib.sprc_stream_cus(h)
    torch.cuda.synchronize()
    L.check(lib.sprc_stream_destroy(h), "sprc_stream_destroy")


@pytest.mark.parametrize("case", G.auto_cases(), ids=[c.name for c in G.auto_cases()])
def test_layout_cases_through_the_peeled_split(partition, case):
    """Automatic dispatch: 256x256 on the first 1024 rows, the remainder on the 64x64 ring, on 128x128 or split over K into caller scratch
    (a sentinel sits behind its 8 x rem x N floats) -- padded ldc, ldr != ldc, an offset or aliased residual.  All rows against float64
    and bit for bit against the contiguous launch on the same stream."""
    _alive()
    stream, ncu = partition
    rem = case.M - G.peel_rows(case.M, case.N, case.K, ncu, op=case.op, out=case.out, resid=case.resid is not None)
    route = G.expected_route(case.M, case.N, case.K, ncu, scratch_floats=8 * rem * case.N if case.scratch else 0, **case.route_args())
    if route != case.kernel:
        pytest.skip(f"{case.name}: a quarter of this device is {ncu} CUs, where the dispatcher takes '{route}', not '{case.kernel}'")
    stats = {}
    bad = G.run_checks(G.Runner(DEV), case, stats, stream=stream)
    assert not bad, "\n".join(bad)
