# -*- coding: utf-8 -*-
"""Low-rank adapters on the MI355X through the real library: the cases of tests/test_emu_lora.py (tests/lora_common.py)."""
import pytest

from tests import lora_common as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib

IDS = ["%dx%d_r%d" % s for s in LC.SHAPES]


def test_op_inputs_unchanged_and_guard_bands_keep_their_bits():
    LC.check_inputs_and_guard_bands(_lib(), DEV)


@pytest.mark.parametrize("i", range(len(LC.SHAPES)), ids=IDS)
def test_op_merge_within_the_derived_bound(i):
    LC.check_merge_bound(_lib(), DEV, i)


@pytest.mark.parametrize("i", range(len(LC.SHAPES)), ids=IDS)
def test_op_project_within_the_derived_bound(i):
    LC.check_project_bound(_lib(), DEV, i)


def test_op_exact_invariants():
    LC.check_exact_invariants(_lib(), DEV)


def test_op_argument_errors():
    LC.check_argument_errors(_lib(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_fresh_adapters_leave_the_pretrained_weights(name):
    LC.check_fresh_adapters(name, _lib(), DEV)


def test_targets():
    LC.check_targets(_lib(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_project_after_a_real_backward(name):
    LC.check_project(name, _lib(), DEV)


@pytest.mark.parametrize("name", LC.GOLDEN)
def test_twenty_adapter_steps(name):
    LC.check_training(name, _lib(), DEV)


def test_one_step_is_the_generic_adam_launch_and_the_guard():
    LC.check_step_bits(_lib(), DEV)


def test_checkpoint_round_trip(tmp_path):
    LC.check_checkpoint(_lib(), DEV, tmp_path)


def test_fold():
    LC.check_fold(_lib(), DEV)


def test_launches():
    LC.check_launches(_lib(), DEV)


def test_projection_follows_the_final_micro_step():
    LC.check_micro_steps(_lib(), DEV)
