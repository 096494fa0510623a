# -*- coding: utf-8 -*-
"""Global-norm gradient clipping and the non-finite-step guard on the host-compiled kernels (tests/clip_common.py holds the cases;
tests/test_gpu_clip.py runs the same ones on the MI355X)."""
import pytest

from tests import clip_common as CC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu
DEV = "cpu"


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_norm_op_level(n, misalign):
    CC.check_norm(emu_library(), DEV, n, misalign)


def test_norm_range():
    CC.check_range(emu_library(), DEV)


@pytest.mark.parametrize("misalign", [0, 1])
def test_nonfinite_detection(misalign):
    CC.check_nonfinite(emu_library(), DEV, misalign)


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["clip_active", "clip_inactive"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_clipped_step_against_torch_op_level(weight_decay, factor):
    CC.check_clipped_step(emu_library(), DEV, weight_decay, factor)


def test_module_level_clipped_training_tiny_k2_up():
    CC.check_module_clipped_training("tiny_k2_up", emu_library(), DEV)


def test_nonfinite_step_is_skipped_and_the_next_one_is_adams_first():
    CC.check_skip(emu_library(), DEV)


def test_guard_off_nan_reaches_the_weights_as_in_torch():
    CC.check_guard_off_nan_reaches_the_weights(emu_library(), DEV)


def test_defaults_are_the_plain_path_bit_for_bit():
    CC.check_defaults(emu_library(), DEV)


def test_guarded_path_launches_and_agreement_with_the_plain_path():
    CC.check_guarded_launches_and_plain_agreement(emu_library(), DEV)


def test_checkpoint_round_trip():
    CC.check_checkpoint(emu_library(), DEV)


def test_autograd_route_and_live_parameters_without_a_gradient():
    CC.check_autograd_route_and_missing_gradients(emu_library(), DEV)
