# -*- coding: utf-8 -*-
"""MI355X: training on padded batches of unequal length (``lengths=``) -- the emulator cases of tests/ragged_common.py on the
device, and the benchmark model at size (B = 8, T = 23040, lengths spread from just above the receptive field to T) against
the oracle on the CPU."""
import pytest

from pytorchwavenetvocoder_amd import _lib
from tests import ragged_common as RG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPE_ARITH = [(s, a) for s in RG.SHAPES for a in RG.FLAG_SETS]
IDS = ["%s-%s" % sa for sa in SHAPE_ARITH]


def _lib_gpu():
    lib = _lib.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("arith", list(RG.FLAG_SETS))
def test_golden_reference_module_gpu(arith):
    RG.check_golden(_lib_gpu(), DEV, arith)


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_vs_oracle_fp64_gpu(shape, arith):
    RG.check_oracle(shape, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_three_loss_routes_agree_gpu(shape):
    RG.check_routes_agree(shape, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape", ["F1", "F2"])
def test_fused_form_is_kept_gpu(shape):
    RG.check_fused_form_kept(shape, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_nothing_existing_moved_gpu(shape, arith):
    RG.check_nothing_moved(shape, arith, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape,arith", SHAPE_ARITH, ids=IDS)
def test_padding_content_does_not_matter_gpu(shape, arith):
    RG.check_padding_content(shape, arith, _lib_gpu(), DEV)


def test_mixture_head_gpu():
    RG.check_mol(_lib_gpu(), DEV)


def test_errors_gpu():
    RG.check_errors(_lib_gpu(), DEV)


def test_benchmark_model_at_size_vs_oracle():
    RG.check_fullsize((256, 80, 64, 256, 10, 3, 2, 80), 8, 23040, 211, _lib_gpu(), DEV)
