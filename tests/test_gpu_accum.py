# -*- coding: utf-8 -*-
"""Gradient accumulation over micro-batches on the MI355X through the real library: the cases of tests/test_emu_accum.py
(tests/accum_common.py)."""
import pytest

from tests import accum_common as AC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("mode", list(AC.MODES))
@pytest.mark.parametrize("misalign", AC.MISALIGN, ids=lambda m: "acc%d_grad%d" % m)
@pytest.mark.parametrize("n", AC.SIZES)
def test_accumulate_op_level(n, misalign, mode):
    AC.check_op(_lib(), DEV, n, misalign, mode)


@pytest.mark.parametrize("misalign", [(1, 1), (2, 3)], ids=lambda m: "acc%d_grad%d" % m)
def test_accumulate_chain_is_the_sum_in_order(misalign):
    AC.check_chain(_lib(), DEV, 4097, misalign)


def test_accumulate_argument_errors():
    AC.check_op_errors(_lib(), DEV)


@pytest.mark.parametrize("split", [(1, 3), (1, 1, 2)], ids=["A2_rows_1_3", "A3_rows_1_1_2"])
def test_module_level_dense(split):
    AC.check_dense(_lib(), DEV, split)


def test_module_level_ragged_with_a_workspace_change():
    AC.check_ragged(_lib(), DEV)


def test_mixture_head_cycle():
    AC.check_mol(_lib(), DEV)


def test_off_means_off():
    AC.check_off_means_off(_lib(), DEV)


def test_norm_is_the_accumulated_gradients():
    AC.check_norm(_lib(), DEV)


def test_nan_in_a_micro_batch_skips_the_step_and_leaks_nothing():
    AC.check_guard(_lib(), DEV)


def test_average_counts_optimizer_steps():
    AC.check_ema_counts_optimizer_steps(_lib(), DEV)


def test_misuse_raises_and_the_engine_recovers():
    AC.check_misuse(_lib(), DEV)


def test_bucket_ranges_tile_the_buffer():
    AC.check_bucket_ranges_tile(_lib(), DEV)
