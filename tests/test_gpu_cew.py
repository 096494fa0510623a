# -*- coding: utf-8 -*-
"""MI355X: the weighted cross-entropy head (class weights, label smoothing, position weights) -- the checkers and gates of
tests/cew_common.py on the device, op level over the full product of Q, option and normalization, each dense and ragged."""
import pytest

from pytorchwavenetvocoder_amd import _lib
from tests import cew_common as CC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_gpu():
    lib = _lib.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("normalize", CC.NORMALIZE)
@pytest.mark.parametrize("option", list(CC.OPTIONS))
@pytest.mark.parametrize("Q", CC.OP_Q)
def test_cew_per_position_gpu(Q, option, normalize):
    CC.check_cew_op(Q, option, normalize, CC.OP_MODES, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", CC.OP_Q)
def test_cew_against_torch_cross_entropy_gpu(Q):
    CC.check_cew_torch(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", CC.MASK_Q)
def test_cew_masked_classes_gpu(Q):
    CC.check_cew_masked(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", CC.OP_Q)
def test_cew_nan_and_inf_stay_in_their_column_gpu(Q):
    CC.check_cew_nonfinite(Q, _lib_gpu(), DEV)


def test_cew_argument_errors_gpu():
    CC.check_cew_errors(_lib_gpu(), DEV)


def test_cew_step_is_the_hand_composed_calls_gpu():
    CC.check_model_composition(_lib_gpu(), DEV)


def test_cew_step_launches_gpu():
    CC.check_model_launches(_lib_gpu(), DEV)


def test_cew_step_with_frozen_parameters_gpu():
    CC.check_model_frozen(_lib_gpu(), DEV)


def test_cew_step_against_fp64_autograd_gpu():
    CC.check_model_numerics(_lib_gpu(), DEV)
