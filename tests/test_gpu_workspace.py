# -*- coding: utf-8 -*-
"""No result depends on what the workspace held before the call, on the MI355X (tests/workspace_common.py): per shape the
pairwise covering of (pre-state, route, arithmetic), the fp16 chain / contraction images before the default arithmetic, each
shape's path, the mid-size model under the default arithmetic, and the decode prefill's workspace."""
import pytest

from tests import workspace_common as WS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = WS.rows()
CASES = [(s, r) for s in WS.SHAPES for r in ROWS]


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("shape,row", CASES, ids=["%s-%s" % (s, WS.row_id(r)) for s, r in CASES])
def test_workspace_independence(shape, row):
    WS.check_workspace_independence(shape, row["route"], row["arith"], row["state"], _lib(), DEV)


@pytest.mark.parametrize("shape", list(WS.SHAPES))
def test_chain_and_mm_f16_images_before_the_default(shape):
    """stale-arith with WN_FLAG_CHAIN_F16PAIR | WN_FLAG_MM_F16PAIR alone in the earlier step (its 16-bit images and maxima)."""
    WS.check_workspace_independence(shape, "train", "default", "stale-arith", _lib(), DEV, stale_flags=WS.CHAIN_MM)


@pytest.mark.parametrize("shape", list(WS.SHAPES))
def test_each_shape_takes_its_path(shape):
    WS.check_path(shape, _lib(), DEV)


@pytest.mark.parametrize("state", ["stale-data", "garbage"])
def test_workspace_independence_midsize(state):
    """The mid-size model (30 fused layers, 256 classes: the loss window starts at column 2944 of 3120) under DEFAULT_FLAGS.
    Loss and weight gradients of the baseline against the oracle step test_gpu_launch_plans' mid-size test uses; dh is compared
    bit for bit only at this size."""
    WS.check_workspace_independence("mid", "train", "default", state, _lib(), DEV, cfg_bt=WS.MIDSIZE)


@pytest.mark.parametrize("name", ["decode_tiny_k2_up", "decode_r64_k2_up"])
def test_decode_prefill_workspace(name):
    WS.check_decode_prefill(name, _lib(), DEV)
