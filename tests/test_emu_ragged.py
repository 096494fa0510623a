# -*- coding: utf-8 -*-
"""CPU-only: training on padded batches of unequal length (``lengths=``) with the kernel sources under the host emulator --
against the reference module's golden values and the fp64 oracle, across the three loss routes, with the fused form kept,
nothing existing moved, the padding's content irrelevant, the mixture head and the error paths (tests/ragged_common.py)."""
import pytest

from tests import ragged_common as RG
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu

SHAPE_ARITH = [(s, a) for s in RG.SHAPES for a in RG.FLAG_SETS]
IDS = ["%s-%s" % sa for sa in SHAPE_ARITH]


@pytest.mark.parametrize("arith", list(RG.FLAG_SETS))
def test_golden_reference_module(arith):
    RG.check_golden(emu_library(), "cpu", arith)


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_vs_oracle_fp64(shape, arith):
    RG.check_oracle(shape, arith, emu_library(), "cpu")


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_three_loss_routes_agree(shape):
    RG.check_routes_agree(shape, emu_library(), "cpu")


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_fused_form_is_kept(shape):
    RG.check_fused_form_kept(shape, emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_nothing_existing_moved(shape, arith):
    RG.check_nothing_moved(shape, arith, emu_library(), "cpu")


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_padding_content_does_not_matter(shape, arith):
    RG.check_padding_content(shape, arith, emu_library(), "cpu")


def test_mixture_head():
    RG.check_mol(emu_library(), "cpu")


def test_errors():
    RG.check_errors(emu_library(), "cpu")
