# -*- coding: utf-8 -*-
"""Training with frozen parameters on the host-compiled kernels (tests/freeze_common.py holds the cases; tests/test_gpu_freeze.py
runs the same ones on the MI355X)."""
import pytest

from tests import clip_common as CC
from tests import freeze_common as FC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu
DEV = "cpu"


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "nan_in_frozen_ranges"])
@pytest.mark.parametrize("name", ["bottom:1", "aux_only", "scatter"])
def test_frozen_parameters_stay_and_trainable_ones_follow_torch(name, poison):
    FC.check_frozen_training(name, emu_library(), DEV, poison=poison)


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_norm_over_ranges_op_level(n, misalign):
    FC.check_norm_live(emu_library(), DEV, n, misalign)


@pytest.mark.parametrize("misalign", [0, 1])
def test_nonfinite_outside_the_ranges_never_skips_inside_always(misalign):
    FC.check_nonfinite_live(emu_library(), DEV, misalign)


@pytest.mark.parametrize("misalign", [0, 1])
@pytest.mark.parametrize("n", CC.SIZES)
def test_adam_over_ranges_op_level(n, misalign):
    FC.check_adam_live(emu_library(), DEV, n, misalign)


def test_argument_errors():
    FC.check_errors(emu_library(), DEV)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_nothing_frozen_is_todays_step_bit_for_bit(guarded):
    FC.check_none_is_todays_step(emu_library(), DEV, guarded)


def test_frozen_sets_take_the_live_launches_and_an_empty_set_none():
    FC.check_frozen_launches(emu_library(), DEV)


def test_freeze_and_train_only():
    FC.check_freeze_and_train_only(emu_library(), DEV)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_changing_the_set_between_steps(guarded):
    FC.check_changing_set(emu_library(), DEV, guarded)


def test_a_skipped_step_trains_nothing():
    FC.check_skipped_step_trains_nothing(emu_library(), DEV)


def test_checkpoint_round_trip_under_a_frozen_set():
    FC.check_checkpoint(emu_library(), DEV)


# The emulator runs a fiber per thread: one plan of a chain shape takes most of a minute here, so each chain shape (P1, P2, P3)
# gets the plan whose check is the strictest (one-layer flush groups: the full pass's bits) under the default arithmetic, and the
# layered path (P4) every plan.  tests/test_gpu_freeze.py runs the whole matrix (4 shapes x 4 plans x 5 freeze sets x 2
# arithmetics), the six-product arithmetic of the chain shapes included, which has no coverage here.
@pytest.mark.parametrize("shape,flag_set,plans", [("P1", "default", ("flush1",)), ("P2", "default", ("flush1",)),
                                                  ("P3", "default", ("flush1",)), ("P4", "default", None),
                                                  ("P4", "six_product", ("flush1", "lpb1"))])
def test_backward_stops_at_the_lowest_trainable_layer(shape, flag_set, plans):
    FC.check_backward_plans(shape, flag_set, emu_library(), DEV, plans=plans)
