# -*- coding: utf-8 -*-
"""MI355X: the soft-target (knowledge distillation) loss head -- the checkers and gates of tests/distill_common.py on the
device, op level over the full product of Q, (alpha, tau) and dense / ragged / full lengths."""
import pytest

from pytorchwavenetvocoder_amd import _lib
from tests import distill_common as DC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_gpu():
    lib = _lib.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("alpha,tau", DC.OP_AT)
@pytest.mark.parametrize("Q", DC.OP_Q)
def test_distill_per_position_gpu(Q, alpha, tau):
    DC.check_distill_op(Q, alpha, tau, DC.OP_MODES, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", DC.MASK_Q)
def test_distill_masked_classes_gpu(Q):
    DC.check_distill_masked(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", DC.OP_Q)
def test_distill_nan_and_inf_stay_in_their_column_gpu(Q):
    DC.check_distill_nonfinite(Q, _lib_gpu(), DEV)


def test_distill_argument_errors_gpu():
    DC.check_distill_errors(_lib_gpu(), DEV)


def test_distill_step_is_the_hand_composed_calls_gpu():
    DC.check_model_composition(_lib_gpu(), DEV)


def test_distill_step_launches_gpu():
    DC.check_model_launches(_lib_gpu(), DEV)


def test_distill_step_with_frozen_parameters_gpu():
    DC.check_model_frozen(_lib_gpu(), DEV)


def test_distill_step_against_fp64_autograd_gpu():
    DC.check_model_numerics(_lib_gpu(), DEV)
