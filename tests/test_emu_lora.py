# -*- coding: utf-8 -*-
"""Low-rank adapters on the host-compiled kernels (tests/lora_common.py holds the cases; tests/test_gpu_lora.py runs the same ones
on the MI355X)."""
import pytest

from tests import lora_common as LC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu
DEV = "cpu"
IDS = ["%dx%d_r%d" % s for s in LC.SHAPES]


def test_op_inputs_unchanged_and_guard_bands_keep_their_bits():
    LC.check_inputs_and_guard_bands(emu_library(), DEV)


@pytest.mark.parametrize("i", range(len(LC.SHAPES)), ids=IDS)
def test_op_merge_within_the_derived_bound(i):
    LC.check_merge_bound(emu_library(), DEV, i)


@pytest.mark.parametrize("i", range(len(LC.SHAPES)), ids=IDS)
def test_op_project_within_the_derived_bound(i):
    LC.check_project_bound(emu_library(), DEV, i)


def test_op_exact_invariants():
    LC.check_exact_invariants(emu_library(), DEV)


def test_op_argument_errors():
    LC.check_argument_errors(emu_library(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_fresh_adapters_leave_the_pretrained_weights(name):
    LC.check_fresh_adapters(name, emu_library(), DEV)


def test_targets():
    LC.check_targets(emu_library(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_project_after_a_real_backward(name):
    LC.check_project(name, emu_library(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_twenty_adapter_steps(name):
    LC.check_training(name, emu_library(), DEV)


def test_one_step_is_the_generic_adam_launch_and_the_guard():
    LC.check_step_bits(emu_library(), DEV)


def test_checkpoint_round_trip(tmp_path):
    LC.check_checkpoint(emu_library(), DEV, tmp_path)


def test_fold():
    LC.check_fold(emu_library(), DEV)


def test_launches():
    LC.check_launches(emu_library(), DEV)


def test_projection_follows_the_final_micro_step():
    LC.check_micro_steps(emu_library(), DEV)
