# -*- coding: utf-8 -*-
"""MI355X: scoring held-out data (``WaveNet.evaluate`` / ``WaveNetEngine.forward_nll``) -- the emulator cases of
tests/eval_common.py on the device."""
import pytest

from pytorchwavenetvocoder_amd import _lib
from tests import eval_common as EV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_gpu():
    lib = _lib.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("shape,arith", EV.SHAPE_ARITH, ids=EV.IDS)
def test_rows_vs_oracle_fp64_gpu(shape, arith):
    EV.check_oracle(shape, arith, _lib_gpu(), DEV)


def test_mixture_head_gpu():
    EV.check_mol(_lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "E1", "P4") for a in EV.FLAG_SETS])
def test_pooled_mean_is_the_training_loss_gpu(shape, arith):
    EV.check_training_loss(shape, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_three_routes_agree_gpu(shape):
    EV.check_routes_agree(shape, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "P3") for a in EV.FLAG_SETS])
def test_nothing_existing_moved_gpu(shape, arith):
    EV.check_nothing_moved(shape, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", [(s, a) for s in EV.WS_CASES for a in EV.FLAG_SETS])
def test_workspace_independence_gpu(shape, arith):
    EV.check_workspace_independence(shape, arith, _lib_gpu(), DEV)


def test_accumulator_three_batches_gpu():
    EV.check_accumulator(_lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", [(s, a) for s in ("F1", "F2", "E1", "P4") for a in EV.FLAG_SETS])
def test_padding_content_does_not_matter_gpu(shape, arith):
    EV.check_padding_content(shape, arith, _lib_gpu(), DEV)


def test_errors_gpu():
    EV.check_errors(_lib_gpu(), DEV)


def test_row_sums_op_gpu():
    EV.check_row_sums_op(_lib_gpu(), DEV)
