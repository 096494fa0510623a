# -*- coding: utf-8 -*-
"""Training with frozen parameters on the MI355X, through the real library: the cases of tests/test_emu_freeze.py
(tests/freeze_common.py), the whole matrix of backward plans, and five steps of a frozen set with the weight gradients on the side
stream, bit-identical from run to run."""
import pytest

from tests import clip_common as CC
from tests import freeze_common as FC
from tests import plan_common as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "nan_in_frozen_ranges"])
@pytest.mark.parametrize("name", ["bottom:1", "aux_only", "scatter"])
def test_frozen_parameters_stay_and_trainable_ones_follow_torch(name, poison):
    FC.check_frozen_training(name, _lib(), DEV, poison=poison)


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_norm_over_ranges_op_level(n, misalign):
    FC.check_norm_live(_lib(), DEV, n, misalign)


@pytest.mark.parametrize("misalign", [0, 1])
def test_nonfinite_outside_the_ranges_never_skips_inside_always(misalign):
    FC.check_nonfinite_live(_lib(), DEV, misalign)


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_adam_over_ranges_op_level(n, misalign):
    FC.check_adam_live(_lib(), DEV, n, misalign)


def test_argument_errors():
    FC.check_errors(_lib(), DEV)


@pytest.mark.parametrize("flag_set", ["default", "six_product"])
@pytest.mark.parametrize("shape", ["P1", "P2", "P3", "P4"])
def test_backward_stops_at_the_lowest_trainable_layer(shape, flag_set):
    FC.check_backward_plans(shape, flag_set, _lib(), DEV)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_nothing_frozen_is_todays_step_bit_for_bit(guarded):
    FC.check_none_is_todays_step(_lib(), DEV, guarded)


def test_frozen_sets_take_the_live_launches_and_an_empty_set_none():
    FC.check_frozen_launches(_lib(), DEV)


def test_freeze_and_train_only():
    FC.check_freeze_and_train_only(_lib(), DEV)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_changing_the_set_between_steps(guarded):
    FC.check_changing_set(_lib(), DEV, guarded)


def test_a_skipped_step_trains_nothing():
    FC.check_skipped_step_trains_nothing(_lib(), DEV)


def test_checkpoint_round_trip_under_a_frozen_set():
    FC.check_checkpoint(_lib(), DEV)


def test_p2_bottom2_with_overlap_five_steps_bit_identical_run_to_run():
    from pytorchwavenetvocoder_amd import _lib as L
    cfg, B, T = PL.SHAPES["P2"]
    FC.check_run_to_run(_lib(), DEV, cfg, B, T, "bottom:2", 4, L.FLAG_BWD_OVERLAP)
