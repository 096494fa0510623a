# -*- coding: utf-8 -*-
"""CPU-only: no result depends on what the workspace held before the call (tests/workspace_common.py), on the host emulator --
shapes P1 (fused, upsampling, aux-fused), P4 (any-size) and N3 (fused, no upsampling layer, ragged tile tails), one arithmetic
each plus the six-product one, each shape's path, and the decode prefill's workspace.

One emulated training step takes 4 - 11 s whatever the shape (single-threaded), so this file runs a hand-picked part of the
matrix -- every pre-state on some shape, NaN (the state no kernel can absorb silently) on all three -- and the cases of one
(shape, route, arithmetic) share their baseline.  Measured: 4 min 44 s in one process on an 8-CPU machine
(profiles/workspace/pytest_emu_workspace.txt).  The pairwise
matrix over every route and arithmetic runs on the MI355X (tests/test_gpu_workspace.py); the emulator's LDS, tile tails and
launch order are not the hardware's."""
import pytest

from tests import workspace_common as WS
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu

# (shape, route, arithmetic, pre-state)
CASES = [
    ("P1", "train", "default", "stale-arith"),
    ("P1", "train", "six", "nan"),
    ("P4", "train", "default", "nan"),
    ("P4", "train0", "default", "garbage"),
    ("P4", "train", "default", "stale-shape"),
    ("P4", "ragged", "six", "stale-data"),
    ("N3", "train", "default+chain16", "nan"),
    ("N3", "train", "default+chain16", "garbage"),
    ("N3", "train", "default+chain16", "stale-arith"),
    ("N3", "full", "six", "stale-data"),
    ("N3", "train", "six", "stale-shape"),
]


@pytest.mark.parametrize("shape,route,arith,state", CASES, ids=["-".join(c).replace("+", "_") for c in CASES])
def test_workspace_independence(shape, route, arith, state):
    WS.check_workspace_independence(shape, route, arith, state, emu_library(), "cpu")


@pytest.mark.parametrize("shape", ["P1", "P4", "N3"])
def test_each_shape_takes_its_path(shape):
    WS.check_path(shape, emu_library(), "cpu")


@pytest.mark.parametrize("name,layered", [("decode_tiny_k2_up", (False, True)), ("decode_r64_k2_up", (False,))],
                         ids=["decode_tiny_k2_up", "decode_r64_k2_up"])
def test_decode_prefill_workspace(name, layered):
    WS.check_decode_prefill(name, emu_library(), "cpu", layered)
