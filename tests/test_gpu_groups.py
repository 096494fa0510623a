# -*- coding: utf-8 -*-
"""Parameter groups in FusedAdam on the MI355X, through the real library: the cases of tests/test_emu_groups.py
(tests/groups_common.py)."""
import pytest

from tests import clip_common as CC
from tests import groups_common as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


def test_group_table_words_and_errors():
    GC.check_group_table(_lib())


@pytest.mark.parametrize("misalign", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1023, 4097])
def test_grouped_adam_is_the_single_group_launch_per_group_bit_for_bit(n, misalign):
    GC.check_adam_groups(_lib(), DEV, n, misalign)


def test_grouped_adam_second_sweep_of_the_grid():
    GC.check_adam_groups(_lib(), DEV, CC.N_BIG, 1)


def test_guarded_scalars_per_group():
    GC.check_guarded_scalars(_lib(), DEV)


def test_argument_errors():
    GC.check_group_call_errors(_lib(), DEV)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded_clip_active"])
def test_decoupled_groups_follow_adamw(guarded):
    GC.check_decoupled(_lib(), DEV, guarded)


def test_decoupled_without_decay_is_l2_without_decay_bit_for_bit():
    GC.check_decoupled_zero_decay_is_l2_zero_decay(_lib(), DEV)


@pytest.mark.parametrize("kw", [dict(), dict(clip=True), dict(ema=True), dict(clip=True, ema=True, freeze=r"\.1\."),
                                dict(freeze=r"\.1\."), dict(scheduler=True), dict(clip=True, scheduler=True),
                                dict(case="tiny_k2_up", clip=True), dict(case="r64_k2_up")],
                         ids=["plain", "clip", "ema", "clip_ema_frozen", "frozen", "step_lr", "clip_step_lr", "golden_clip",
                              "golden_r64"])
def test_module_level_groups_follow_torch_param_groups(kw):
    GC.check_module(_lib(), DEV, **kw)


def test_without_groups_the_optimizer_is_todays():
    GC.check_without_groups_is_todays_optimizer(_lib(), DEV)


def test_constructor_rules():
    GC.check_constructor(_lib(), DEV)


def test_checkpoint_round_trip_through_torch_param_groups():
    GC.check_checkpoint(_lib(), DEV)
