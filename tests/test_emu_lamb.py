# -*- coding: utf-8 -*-
"""Layer-wise adaptive steps (LAMB) and per-tensor norms on the host-compiled kernels (tests/lamb_common.py holds the cases;
tests/test_gpu_lamb.py runs the same ones on the MI355X)."""
import pytest

from tests import lamb_common as LC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu
DEV = "cpu"

MODULE_CASES = [dict(), dict(clip=True), dict(ema=True), dict(clip=True, ema=True, freeze=r"\.1\."),
                dict(groups=LC.GROUPS, scheduler=True), dict(accum=True), dict(clip=True, groups=LC.GROUPS, max_trust=0.5),
                dict(case="tiny_k2_up", clip=True)]
MODULE_IDS = ["plain", "clip", "ema", "clip_ema_frozen", "groups_step_lr", "accumulation", "clip_groups_max_trust", "golden_clip"]


def test_tensor_table_words_and_errors():
    LC.check_tensor_table(emu_library())


@pytest.mark.parametrize("misalign", [0, 1, 2, 3, (0, 1, 1, 2, 3)], ids=["0", "1", "2", "3", "mixed"])
@pytest.mark.parametrize("t", [1, 1000])
def test_lamb_step_against_fp64_and_the_grouped_adam_bits(t, misalign):
    LC.check_lamb_step(emu_library(), DEV, "chunks", misalign, t=t)


def test_lamb_step_over_1100_tensors():
    LC.check_lamb_step(emu_library(), DEV, "many", 1, variants=("plain", "guarded_ema"))


def test_max_trust_ratio_clamps_exactly_to_min():
    LC.check_lamb_step(emu_library(), DEV, "chunks", 3, variants=("plain", "guarded_ema"), max_trust=2.0)


def test_guarded_step_with_a_nan_gradient_writes_nothing():
    LC.check_guard_writes_nothing(emu_library(), DEV)


def test_zero_rules():
    LC.check_zero_rules(emu_library(), DEV)


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
@pytest.mark.parametrize("layout", ["chunks", "many"])
def test_tensor_sumsq_against_numpy_fp64(layout, misalign):
    LC.check_tensor_sumsq(emu_library(), DEV, layout, misalign)


def test_argument_errors():
    LC.check_call_errors(emu_library(), DEV)


@pytest.mark.parametrize("kw", MODULE_CASES, ids=MODULE_IDS)
def test_module_level_steps_follow_the_fp64_reference(kw):
    LC.check_module(emu_library(), DEV, **kw)


def test_default_adaptation_by_shape_and_group_override():
    LC.check_default_adaptation_by_shape(emu_library(), DEV)


def test_layer_adaptation_off_is_todays_optimizer():
    LC.check_off_is_todays_optimizer(emu_library(), DEV)


def test_checkpoint_round_trip_through_adam():
    LC.check_checkpoint(emu_library(), DEV)


def test_changed_trainable_set_rebuilds_the_table_once():
    LC.check_changed_set_rebuilds_the_table_once(emu_library(), DEV)


def test_constructor_rules():
    LC.check_constructor(emu_library(), DEV)
