# -*- coding: utf-8 -*-
"""wn_op_gemm (csrc/wn_gemm.hip) op-level on the MI355X: the matrix of tests/gemm_common.py through the gfx950 library on
the current stream -- every operand mode, staging path and epilogue, bit-equal to the fp64 restatement of
include/wavenet_hip_gemm.h with small-integer operands and inside the derived forward error bound with normal ones.
Every operand lies between NaN guard bands inside one allocation: an over-read cannot fault, it shows as NaN."""
import pytest

from tests import gemm_common as GC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("data", ["exact", "rounded"])
@pytest.mark.parametrize("name", GC.CASE_NAMES)
def test_matrix(name, data):
    ratio = GC.run_case(_lib(), DEV, GC.CASE_BY_NAME[name], data)
    print("%s/%s: worst error / bound %.3f" % (name, data, ratio))
