"""Every fused GEMM epilogue on every kernel variant against the fp64 reference of tests/_gemm_ref.py: each
Python-reachable EPI_* code x four operand layouts x both C / mask / bias / colsum layouts (vector body + scalar
tail, all scalar) at the tile, tail and stride edges, plus split-K (in-kernel atomics, both slab reduces), the
batched mode with a bias and one gaussian-data case per layout. Exact-regime outputs must be bit-equal to the
RNE-rounded reference, every NaN padding element must survive. The three LDS-DMA tiles run in this process
through ops.gemm(tile=); the register-staged v1 kernel (the > 2 GiB operand fallback) is forced by
MINIPS_GEMM_TILE=1, which is read once per process, so it runs in one fresh child."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _gemm_ref as G
from minips_amd import _native, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "import sys; sys.path.insert(0, 'tests'); import _gemm_ref; _gemm_ref.child_main()"
_broken = []  # a variant that raised (device fault, child abort / timeout): nothing more is started on the device


def _report(variant, fails, stats):
    print(f"gemm epilogues {variant}: {stats}")
    assert stats["cells"] >= 16 * (2 * 11 + 1) + 4 + 5 + 1, stats
    assert not fails, (variant, len(fails), fails[:12])


@pytest.mark.parametrize("tile", [128, 200, 256])
def test_epilogues_v2_tile(dev, tile):
    if _broken:
        pytest.fail(f"not run: {_broken[0]} did not finish")
    _native.kernels()
    try:
        fails, stats = G.run_variant(ops, dev, tile)
        torch.cuda.synchronize()
    except BaseException:
        _broken.append(f"tile {tile}")
        raise
    _report(f"v2 tile {tile}", fails, stats)


def test_epilogues_v1_register_staged(dev):
    if _broken:
        pytest.fail(f"not run: {_broken[0]} did not finish")
    env = {k: v for k, v in os.environ.items() if k != "MINIPS_GEMM_TILE"}
    env["MINIPS_GEMM_TILE"] = "1"
    try:
        r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=240)
    except subprocess.TimeoutExpired:
        _broken.append("the v1 child")
        raise
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode not in (0, 1) or not lines:
        _broken.append("the v1 child")
        pytest.fail(f"v1 child exit {r.returncode}: {r.stdout[-2000:]} {r.stderr[-3000:]}")
    res = json.loads(lines[-1])
    _report("v1", res["fails"], res["stats"])
    assert r.returncode == 0 and res["nfails"] == 0
