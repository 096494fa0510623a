# -*- coding: utf-8 -*-
"""CPU-only: scoring held-out data (``WaveNet.evaluate`` / ``WaveNetEngine.forward_nll`` and the C entry points behind them)
with the kernel sources under the host emulator -- against the fp64 oracle, the training loss and across the three routes,
with nothing of the training step moved, independent of the workspace's and the padding's content, the accumulator, the
error paths and the reduction kernel at op level (tests/eval_common.py)."""
import pytest

from tests import eval_common as EV
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("shape,arith", EV.SHAPE_ARITH, ids=EV.IDS)
def test_rows_vs_oracle_fp64(shape, arith):
    EV.check_oracle(shape, arith, emu_library(), "cpu")


def test_mixture_head():
    EV.check_mol(emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "E1", "P4") for a in EV.FLAG_SETS])
def test_pooled_mean_is_the_training_loss(shape, arith):
    EV.check_training_loss(shape, arith, emu_library(), "cpu")


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_three_routes_agree(shape):
    EV.check_routes_agree(shape, emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "P3") for a in EV.FLAG_SETS])
def test_nothing_existing_moved(shape, arith):
    EV.check_nothing_moved(shape, arith, emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", [(s, a) for s in EV.WS_CASES for a in EV.FLAG_SETS])
def test_workspace_independence(shape, arith):
    EV.check_workspace_independence(shape, arith, emu_library(), "cpu")


def test_accumulator_three_batches():
    EV.check_accumulator(emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "F2", "E1", "P4") for a in EV.FLAG_SETS])
def test_padding_content_does_not_matter(shape, arith):
    EV.check_padding_content(shape, arith, emu_library(), "cpu")


def test_errors():
    EV.check_errors(emu_library(), "cpu")


def test_row_sums_op():
    EV.check_row_sums_op(emu_library(), "cpu")
