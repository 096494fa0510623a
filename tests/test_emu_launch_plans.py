# -*- coding: utf-8 -*-
"""CPU-only: backward launch plans under every arithmetic on the host emulator (tests/plan_common.py) -- the pairwise plan
matrix on four shapes, each shape's own path, and the guards that keep a backward call consistent with its forward."""
import ctypes

import pytest
import torch

from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS, WaveNetEngine, _ptr, load_state_into_flat
from tests import plan_common as PL
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu

ROWS = PL.pairwise_rows()
CASES = [(s, r) for s in PL.SHAPES for r in ROWS]


@pytest.mark.parametrize("shape,row", CASES, ids=["%s-%s" % (s, PL.row_id(r)) for s, r in CASES])
def test_launch_plan_matrix(shape, row):
    cfg, B, T = PL.SHAPES[shape]
    flags = PL.row_flags(row, cfg[4] * cfg[5])
    PL.check_plan(cfg, B, T, PL.SEED, emu_library(), "cpu", flags, row["lpb"], row["t_first"], row["scale"])


@pytest.mark.parametrize("shape", list(PL.SHAPES))
def test_each_shape_takes_its_path(shape):
    """Under DEFAULT_FLAGS and the default plan each shape launches what it is in the matrix for (a change of a dispatch rule
    must not silently take a path out of the matrix)."""
    cfg, B, T = PL.SHAPES[shape]
    _, _, _, log = PL.check_plan(cfg, B, T, PL.SEED, emu_library(), "cpu", DEFAULT_FLAGS, 0, "rf", "ws", want_log=True)
    need, never = PL.PATH_TAGS[shape]
    for tag in need:
        assert log.get(tag, 0) >= 1, (shape, tag, log)
    for tag in never:
        assert tag not in log, (shape, tag, log)


FAMILY = {"NO_FUSED": _lib.FLAG_NO_FUSED, "EXACT_MFMA": _lib.FLAG_EXACT_MFMA,
          "MM_F16PAIR": _lib.FLAG_MM_F16PAIR, "CHAIN_F16PAIR": _lib.FLAG_CHAIN_F16PAIR}


@pytest.mark.parametrize("bit", list(FAMILY))
def test_kernel_family_change_since_the_forward(bit):
    """engine.flags toggled between forward_loss and backward.  NO_FUSED / EXACT_MFMA change the activations the forward saves
    (the fused forward saves no Gt): backward raises with and without repack=True.  MM_F16PAIR / CHAIN_F16PAIR change only the
    weight images: backward raises, repack=True rebuilds them and the gradients meet the oracle's gates."""
    cfg, B, T = PL.SHAPES["P1"]
    params, x, h, t, _, _, grads_ref = PL.reference(cfg, B, T, PL.SEED)
    eng = WaveNetEngine(*cfg, device="cpu", library=emu_library())
    eng.flags = DEFAULT_FLAGS
    load_state_into_flat(eng, params)
    _, dl = eng.forward_loss(x, h, t)
    eng.flags ^= FAMILY[bit]
    with pytest.raises(_lib.WnError):
        eng.backward(dl)
    if bit in ("NO_FUSED", "EXACT_MFMA"):
        with pytest.raises(_lib.WnError):
            eng.backward(dl, repack=True)
    else:
        eng.grads().fill_(float("nan"))
        PL.check_grads(eng, eng.backward(dl, repack=True).clone(), cfg, grads_ref, "%s toggled, repack" % bit)


def test_amax_word_after_a_forward_without_loss_call():
    """WN_FLAG_DW_F16_AMAX_WS through the C ABI: the maximum a loss call left in the workspace belongs to that call's gradient.
    After forward_loss(dl1) and a plain wn_forward, a backward of dl2 = dl1 * 2^-40 with the flag has no measured maximum: the
    six-product redo is forced (include/wavenet_hip.h), the result is the six-product call's own, bit for bit -- not dl1's
    scale applied to dl2 (which puts dl2 below fp16's range)."""
    cfg, B, T = PL.SHAPES["P1"]
    params, x, h, t, _, _, grads_ref = PL.reference(cfg, B, T, PL.SEED)
    eng = WaveNetEngine(*cfg, device="cpu", library=emu_library())
    eng.flags = DEFAULT_FLAGS
    load_state_into_flat(eng, params)
    _, dl1 = eng.forward_loss(x, h, t)
    eng.forward(x, h)
    dl2 = dl1 * 2.0 ** -40
    rf = eng.receptive_field
    ws = eng.workspace(B, T)
    xc, hc = eng._last_inputs

    def call(flags):
        g = torch.full_like(eng.grads(), float("nan"))
        rc = eng.lib.wn_backward_window(ctypes.byref(eng.cfg), B, T, _ptr(eng.flat_params), _ptr(xc), _ptr(hc), _ptr(dl2), rf,
                                        _ptr(g), _ptr(ws), ws.numel() * 4, None, 0, 0, flags, None)
        eng.lib.check(rc, "wn_backward_window")
        return g
    g_ws = call(DEFAULT_FLAGS | _lib.FLAG_DW_F16_AMAX_WS)
    g_six = call(SIX_PRODUCT_FLAGS)
    scaled = {k: (None if v is None else v * 2.0 ** -40) for k, v in grads_ref.items()}
    PL.check_grads(eng, g_six, cfg, scaled, "six products")
    PL.check_grads(eng, g_ws, cfg, scaled, "AMAX_WS without a loss call")
    assert torch.equal(g_ws, g_six)
