# -*- coding: utf-8 -*-
"""The exponential moving average of the weights in the Adam launch, and the in-place swap, on the host-compiled kernels
(tests/ema_common.py holds the cases; tests/test_gpu_ema.py runs the same ones on the MI355X)."""
import pytest

from tests import ema_common as EC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu
DEV = "cpu"


@pytest.mark.parametrize("misalign", EC.SWAP_MISALIGN, ids=lambda m: "a%d_b%d" % m)
@pytest.mark.parametrize("n", EC.SWAP_SIZES)
def test_swap_op_level(n, misalign):
    EC.check_swap(emu_library(), DEV, n, misalign)


def test_swap_refuses_overlapping_ranges():
    EC.check_swap_errors(emu_library(), DEV)


@pytest.mark.parametrize("ema_decay,warmup,t", EC.RECURRENCE_CASES)
def test_recurrence_in_isolation(ema_decay, warmup, t):
    EC.check_recurrence(emu_library(), DEV, ema_decay, warmup, t)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
def test_ema_on_changes_nothing_else(weight_decay, guarded):
    EC.check_ema_changes_nothing_else(emu_library(), DEV, weight_decay, guarded)


def test_module_level_against_torch_tiny_k2_up():
    EC.check_module_ema_training("tiny_k2_up", emu_library(), DEV)


def test_skipped_step_leaves_the_average_and_the_warmup_index():
    EC.check_guard(emu_library(), DEV)


def test_launches():
    EC.check_launches(emu_library(), DEV)


def test_ema_weights_block():
    EC.check_ema_weights(emu_library(), DEV)


def test_checkpoint_round_trip(tmp_path):
    EC.check_checkpoint(emu_library(), DEV, tmp_path)


def test_entry_point_argument_errors():
    EC.check_api_errors(emu_library(), DEV)
