# -*- coding: utf-8 -*-
"""Op-level checks of the generic f32-MFMA contraction (csrc/wn_gemm.hip) through wn_op_gemm, kernel
sources under the host emulator: dW-type (k = time) with split-K, segments + shifts (16-byte and
scalar staging paths), one-hot operand, row sums; and the op-level matrix of tests/gemm_common.py (both operand modes, every
staging path and epilogue input, guard bands) with its coverage test and the argument checks."""
import ctypes

import pytest
import torch

from pytorchwavenetvocoder_amd import _lib as L
from tests import gemm_common as GC
from tests.emu_util import emu_library
from tests.gemm_util import check_dw_type

pytestmark = pytest.mark.emu


@pytest.mark.parametrize("kw", [
    dict(M=64, N=64, T=1000, B=2, ksplit=4),                                        # aligned -> 16-byte loads
    dict(M=128, N=128, T=1000, B=1, ksplit=3, seg_len=64, shift0=4, shift_step=-4),  # two taps, shift 4 / 0
    dict(M=128, N=128, T=600, B=1, ksplit=2, seg_len=64, shift0=1, shift_step=-1),   # shift 1 -> scalar path
    dict(M=70, N=50, T=333, B=2, ksplit=2),                                          # ragged everything
    dict(M=64, N=512, T=1500, B=1, ksplit=6, onehot_Q=256, shift0=1, shift_step=-1),
    dict(M=64, N=74, T=700, B=2, ksplit=3, onehot_Q=37, shift0=1, shift_step=-1),
])
def test_dw_type(kw):
    err, rerr = check_dw_type(emu_library(), "cpu", **kw)
    assert err <= 2e-6, err
    assert rerr <= 1e-4, rerr


# ---- the op-level matrix (tests/gemm_common.py): every operand mode, staging path and epilogue ---------------------
@pytest.mark.parametrize("data", ["exact", "rounded"])
@pytest.mark.parametrize("name", GC.CASE_NAMES)
def test_matrix(name, data):
    """exact: bit-equal to the fp64 restatement of the header; rounded: inside the derived forward error bound.  Guard
    bands are NaN, so a read outside an operand fails either mode; a store outside C / a_rowsum fails the sentinel check.
    Two broken contracts change no value and end the process instead of failing an assertion: a misaligned 16-byte access
    (SIGILL, the alignment trap of tests/emu/build_emu.py) and a read past the fenced A of w_ragged_m_65_fenced (SIGSEGV).
    pytest's fault handler then prints this test's traceback, and pytest-xdist names the case its worker crashed in."""
    ratio = GC.run_case(emu_library(), "cpu", GC.CASE_BY_NAME[name], data)
    print("%s/%s: worst error / bound %.3f" % (name, data, ratio))


def test_matrix_reaches_every_path_and_variant():
    cov = GC.coverage()
    assert set(cov) == GC.ALL_LABELS, (sorted(GC.ALL_LABELS - set(cov)), sorted(set(cov) - GC.ALL_LABELS))
    assert sum(1 for lab in cov if lab.startswith("variant(")) == 12
    # no staging-path label hangs only on cases whose relu / b_relu would turn a NaN of the guard band into 0
    soft = {c["name"] for c in GC.CASES if c.get("relu") or c.get("b_relu")}
    for lab, names in cov.items():
        if lab not in GC.EPILOGUE and not lab.startswith("variant("):
            assert set(names) - soft, lab


@pytest.mark.parametrize("bad", [
    dict(M=0), dict(M=-1), dict(a_kmajor=1, b_kmajor=0), dict(a_kmajor=0, b_kmajor=1), dict(b_seg_len=0), dict(b_seg_len=-64),
    dict(kchunk=0), dict(kchunk=-32), dict(onehot=True),
], ids=lambda b: "-".join("%s=%s" % kv for kv in b.items()))
def test_rejected_arguments_launch_nothing(bad):
    """wn_op_gemm returns non-zero and leaves C untouched (every launch of a valid shape stores all of C, so an untouched
    C is no launch).  A one-hot operand exists for the dW (k = time) mode only."""
    lib = emu_library()
    M = N = K = 64
    A, B = torch.ones(K, M), torch.ones(K, N)
    idx = torch.zeros(N, dtype=torch.int64)
    C = torch.full((M, N), -7.0)
    g = L.WnGemmArgs.default()
    g.M, g.N, g.K = M, N, K
    g.A, g.lda, g.B, g.ldb, g.b_clen = A.data_ptr(), M, B.data_ptr(), N, N
    g.C, g.ldc = C.data_ptr(), N
    for k, v in bad.items():
        if k == "onehot":
            g.b_index, g.b_index_mod, g.b_seg_len = idx.data_ptr(), 64, 64
        else:
            setattr(g, k, v)
    rc = lib.wn_op_gemm(ctypes.byref(g), None)
    assert rc != 0
    assert lib.wn_last_error()                      # the reason is reported
    assert bool((C == -7.0).all())
    # the same block without the bad field is accepted (the rejection above was that field's)
    g2 = L.WnGemmArgs.default()
    g2.M, g2.N, g2.K = M, N, K
    g2.A, g2.lda, g2.B, g2.ldb, g2.b_clen = A.data_ptr(), M, B.data_ptr(), N, N
    g2.C, g2.ldc = C.data_ptr(), N
    assert lib.wn_op_gemm(ctypes.byref(g2), None) == 0
    assert bool((C == float(K)).all())
