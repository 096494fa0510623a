# -*- coding: utf-8 -*-
"""CPU-only: the soft-target (knowledge distillation) loss head with the kernel sources under the host emulator
(tests/distill_common.py): k_softmax_distill at op level on a subset that visits every Q, every (alpha, tau), dense and ragged;
masked classes, non-finite inputs, argument errors; WaveNet.loss_and_backward(teacher_logits=...) at model level."""
import pytest

from tests import distill_common as DC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("Q,alpha,tau,modes", DC.EMU_MATRIX, ids=["%d-%g-%g-%s" % (m[0], m[1], m[2], "+".join(m[3])) for m in DC.EMU_MATRIX])
def test_distill_per_position(Q, alpha, tau, modes):
    DC.check_distill_op(Q, alpha, tau, modes, emu_library(), "cpu")


@pytest.mark.parametrize("Q", DC.MASK_Q)
def test_distill_masked_classes(Q):
    DC.check_distill_masked(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q", (37, 300))
def test_distill_nan_and_inf_stay_in_their_column(Q):
    DC.check_distill_nonfinite(Q, emu_library(), "cpu")


def test_distill_argument_errors():
    DC.check_distill_errors(emu_library(), "cpu")


def test_distill_step_is_the_hand_composed_calls():
    DC.check_model_composition(emu_library(), "cpu")


def test_distill_step_launches():
    DC.check_model_launches(emu_library(), "cpu")


def test_distill_step_with_frozen_parameters():
    DC.check_model_frozen(emu_library(), "cpu")


def test_distill_step_against_fp64_autograd():
    DC.check_model_numerics(emu_library(), "cpu")
