# -*- coding: utf-8 -*-
"""MI355X: the loss heads per position at trained-model logits against fp64 -- the checkers and gates of
tests/loss_common.py on the device, the fused epilogue over the full product of configurations, arithmetics and cases."""
import pytest

from pytorchwavenetvocoder_amd import _lib
from tests import loss_common as LC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_gpu():
    lib = _lib.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_per_position_gpu(Q):
    LC.check_softmax_op(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_masked_target_gpu(Q):
    LC.check_softmax_masked_target(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", LC.OP_Q)
def test_softmax_head_nan_and_inf_stay_in_their_column_gpu(Q):
    LC.check_softmax_nonfinite(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q,arith,case", LC.FUSED_MATRIX, ids=["%d-%s-%s" % m for m in LC.FUSED_MATRIX])
def test_fused_epilogue_per_position_gpu(Q, arith, case):
    LC.check_fused(Q, arith, case, _lib_gpu(), DEV).report("fused Q=%d %s %s" % (Q, arith, case))


@pytest.mark.parametrize("Q,arith", [(Q, a) for Q in LC.FUSED_CONFIGS for a in LC.FUSED_FLAGS])
def test_fused_epilogue_invariants_gpu(Q, arith):
    LC.check_fused_invariants(Q, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q,arith", [(Q, a) for Q in LC.FUSED_CONFIGS for a in LC.FUSED_FLAGS])
def test_fused_epilogue_masked_target_gpu(Q, arith):
    LC.check_fused_masked_target(Q, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("Q", list(LC.FUSED_CONFIGS))
def test_fused_epilogue_in_the_redo_launch_gpu(Q):
    LC.check_fused_redo(Q, _lib_gpu(), DEV)


@pytest.mark.parametrize("num_classes,nm,regime", LC.MOL_MATRIX)
def test_mixture_head_per_element_gpu(num_classes, nm, regime):
    LC.check_mol_op(num_classes, nm, regime, _lib_gpu(), DEV)
