# -*- coding: utf-8 -*-
"""CPU-only: the weighted cross-entropy head (class weights, label smoothing, position weights) with the kernel sources under the
host emulator (tests/cew_common.py): k_softmax_cew, k_softmax_cew_wide, k_ce_divisor and k_cew_reduce at op level on a subset
that visits every Q, every option, both normalizations, dense and ragged; torch's own criterion; masked classes, non-finite
inputs, argument errors; WaveNet.loss_and_backward(class_weights=, label_smoothing=, position_weights=, normalize=) at model
level."""
import pytest

from tests import cew_common as CC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


def test_cew_inputs_self_check():
    CC.self_check()


@pytest.mark.parametrize("Q,option,normalize,modes", CC.EMU_MATRIX, ids=["%d-%s-%s-%s" % (m[0], m[1], m[2], "+".join(m[3])) for m in CC.EMU_MATRIX])
def test_cew_per_position(Q, option, normalize, modes):
    CC.check_cew_op(Q, option, normalize, modes, emu_library(), "cpu")


@pytest.mark.parametrize("Q", (37, 300))
def test_cew_against_torch_cross_entropy(Q):
    CC.check_cew_torch(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q", (37, 300))
def test_cew_masked_classes(Q):
    CC.check_cew_masked(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q", (37, 300))
def test_cew_nan_and_inf_stay_in_their_column(Q):
    CC.check_cew_nonfinite(Q, emu_library(), "cpu")


def test_cew_argument_errors():
    CC.check_cew_errors(emu_library(), "cpu")


def test_cew_step_is_the_hand_composed_calls():
    CC.check_model_composition(emu_library(), "cpu", option_sets=1)


def test_cew_step_launches():
    CC.check_model_launches(emu_library(), "cpu")


def test_cew_step_with_frozen_parameters():
    CC.check_model_frozen(emu_library(), "cpu")


def test_cew_step_against_fp64_autograd():
    CC.check_model_numerics(emu_library(), "cpu")
