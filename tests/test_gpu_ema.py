# -*- coding: utf-8 -*-
"""The exponential moving average of the weights in the Adam launch, and the in-place swap, on the MI355X through the real library:
the cases of tests/test_emu_ema.py (tests/ema_common.py) and the second golden case."""
import pytest

from tests import ema_common as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("misalign", EC.SWAP_MISALIGN, ids=lambda m: "a%d_b%d" % m)
@pytest.mark.parametrize("n", EC.SWAP_SIZES)
def test_swap_op_level(n, misalign):
    EC.check_swap(_lib(), DEV, n, misalign)


def test_swap_refuses_overlapping_ranges():
    EC.check_swap_errors(_lib(), DEV)


@pytest.mark.parametrize("ema_decay,warmup,t", EC.RECURRENCE_CASES)
def test_recurrence_in_isolation(ema_decay, warmup, t):
    EC.check_recurrence(_lib(), DEV, ema_decay, warmup, t)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_ema_on_changes_nothing_else(weight_decay, guarded):
    EC.check_ema_changes_nothing_else(_lib(), DEV, weight_decay, guarded)


@pytest.mark.parametrize("name", ["tiny_k2_up", "r64_k2_up"])
def test_module_level_against_torch(name):
    EC.check_module_ema_training(name, _lib(), DEV)


def test_skipped_step_leaves_the_average_and_the_warmup_index():
    EC.check_guard(_lib(), DEV)


def test_launches():
    EC.check_launches(_lib(), DEV)


def test_ema_weights_block():
    EC.check_ema_weights(_lib(), DEV)


def test_checkpoint_round_trip(tmp_path):
    EC.check_checkpoint(_lib(), DEV, tmp_path)


def test_entry_point_argument_errors():
    EC.check_api_errors(_lib(), DEV)
