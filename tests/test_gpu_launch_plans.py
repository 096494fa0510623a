# -*- coding: utf-8 -*-
"""Backward launch plans under every arithmetic on the MI355X: the pairwise plan matrix of tests/plan_common.py (the same rows
as tests/test_emu_launch_plans.py, the side-stream plans on a real second stream), and the overlap properties of the mid-size
model under the DEFAULT arithmetic."""
import pytest
import torch

from tests import plan_common as PL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = PL.pairwise_rows()
CASES = [(s, r) for s in PL.SHAPES for r in ROWS]


def _lib():
    from pytorchwavenetvocoder_amd import _lib as L
    lib = L.load_library()
    assert not lib.is_emulator
    return lib


@pytest.mark.parametrize("shape,row", CASES, ids=["%s-%s" % (s, PL.row_id(r)) for s, r in CASES])
def test_launch_plan_matrix(shape, row):
    cfg, B, T = PL.SHAPES[shape]
    flags = PL.row_flags(row, cfg[4] * cfg[5])
    PL.check_plan(cfg, B, T, PL.SEED, _lib(), DEV, flags, row["lpb"], row["t_first"], row["scale"])


@pytest.mark.parametrize("shape", list(PL.SHAPES))
def test_each_shape_takes_its_path(shape):
    cfg, B, T = PL.SHAPES[shape]
    _, _, _, log = PL.check_plan(cfg, B, T, PL.SEED, _lib(), DEV, PL.DEFAULT_FLAGS, 0, "rf", "ws", want_log=True)
    need, never = PL.PATH_TAGS[shape]
    for tag in need:
        assert log.get(tag, 0) >= 1, (shape, tag, log)
    for tag in never:
        assert tag not in log, (shape, tag, log)


def test_overlap_and_flush_properties_midsize_default_arithmetic():
    """test_gpu_parity.test_stream_overlap_modes_midsize's properties under DEFAULT_FLAGS (fp16 pair splits: one overflow
    word per workspace, read by the fp16 launches of both streams) on the training step's calls (forward_loss, backward over
    the loss window), the gradient buffer NaN before every backward:
      * for one launch-group size (WN_FLAG_DW_FLUSH) serial and WN_FLAG_BWD_OVERLAP give bit-identical gradients, and each is
        bit-identical run to run, for every bucket size;
      * different group sizes agree within 1e-5 of the maximum;
      * every run meets the oracle's gradient gates."""
    from pytorchwavenetvocoder_amd import _lib as L
    from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, load_state_into_flat
    cfg_t = (256, 80, 64, 256, 10, 3, 2, 80)
    B, T = 2, 3120
    params, x, h, t, loss_ref, _, grads_ref = PL.reference(cfg_t, B, T, 41, scale=0.05)
    x, h, t = x.to(DEV), h.to(DEV), t.to(DEV)
    worst = {}

    def run(flags, lpb, arith="default"):
        eng = WaveNetEngine(*cfg_t, device=DEV, library=_lib())
        eng.flags = flags
        load_state_into_flat(eng, params)
        out = []
        for rep in range(2):
            loss, dl = eng.forward_loss(x, h, t)
            assert abs(float(loss.cpu()) - float(loss_ref)) <= 1e-5
            eng.grads().fill_(float("nan"))
            g = eng.backward(dl, layers_per_bucket=lpb).clone()
            torch.cuda.synchronize()
            out.append(g)
        assert torch.equal(out[0], out[1]), "run to run (flags %#x, lpb %d)" % (flags, lpb)
        e, k = PL.check_grads(eng, out[0].cpu(), cfg_t, grads_ref, "flags %#x lpb %d" % (flags, lpb))
        if e > worst.get(arith, (0.0, None))[0]:
            worst[arith] = (e, k)
        return out[0]

    base = run(DEFAULT_FLAGS, 0)
    for n in (1, 2, 5, 30):
        F = DEFAULT_FLAGS | L.flag_dw_flush(n)
        for lpb in (0, 1, 7, 10):
            serial = run(F, lpb)
            over = run(F | L.FLAG_BWD_OVERLAP, lpb)
            assert torch.equal(serial, over), "side-stream weight gradients differ from the serial ones (flush %d, lpb %d)" % (n, lpb)
            d = float((serial - base).abs().max())
            assert d <= 1e-5 * float(base.abs().max()), "flush %d lpb %d: %g from the one-group plan" % (n, lpb, d)
    run(SIX_PRODUCT_FLAGS, 0, "six")
    run(SIX_PRODUCT_FLAGS | L.FLAG_BWD_OVERLAP | L.flag_dw_flush(5), 7, "six")
    for a, (e, k) in sorted(worst.items()):
        print("mid-size worst gradient rel err, %s arithmetic: %.3g (%s)" % (a, e, k))
