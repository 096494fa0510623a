# -*- coding: utf-8 -*-
"""CPU-only: the loss heads per position at trained-model logits against fp64, with the kernel sources under the host
emulator (tests/loss_common.py): k_softmax_ce at op level, the cross-entropy epilogue of conv_post_2 through the head's
parameters (six-product and fp16-pair instantiation, and the conditional redo launch), k_mol_nll at op level."""
import pytest

from tests import loss_common as LC
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_per_position(Q):
    LC.check_softmax_op(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_masked_target(Q):
    LC.check_softmax_masked_target(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_nan_and_inf_stay_in_their_column(Q):
    LC.check_softmax_nonfinite(Q, emu_library(), "cpu")


@pytest.mark.parametrize("Q,arith,case", LC.FUSED_MATRIX_EMU, ids=["%d-%s-%s" % m for m in LC.FUSED_MATRIX_EMU])
def test_fused_epilogue_per_position(Q, arith, case):
    """(F3, a bias of +-3e4 on every class, is the case that made the epilogue form its loss as (max - v_t) + log(s):
    profiles/loss_heads/NOTES.md.)"""
    LC.check_fused(Q, arith, case, emu_library(), "cpu").report("fused Q=%d %s %s" % (Q, arith, case))


@pytest.mark.parametrize("Q,arith", [(256, "default"), (130, "six")])
def test_fused_epilogue_invariants(Q, arith):
    LC.check_fused_invariants(Q, arith, emu_library(), "cpu")


@pytest.mark.parametrize("Q,arith", [(200, "default")])
def test_fused_epilogue_masked_target(Q, arith):
    LC.check_fused_masked_target(Q, arith, emu_library(), "cpu")


@pytest.mark.parametrize("Q", [200])
def test_fused_epilogue_in_the_redo_launch(Q):
    LC.check_fused_redo(Q, emu_library(), "cpu")


@pytest.mark.parametrize("num_classes,nm,regime", LC.MOL_MATRIX)
def test_mixture_head_per_element(num_classes, nm, regime):
    LC.check_mol_op(num_classes, nm, regime, emu_library(), "cpu")
