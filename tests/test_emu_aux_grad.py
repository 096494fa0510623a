# -*- coding: utf-8 -*-
"""CPU-only: the gradient with respect to the aux features (dL/dh, wn_backward_dh) on the host emulator -- through autograd
against the reference module's golden values and the oracle, under the backward launch plans of tests/plan_common.py, bit for bit
across the knobs that leave dP unchanged, and the frozen-model call (no weight-gradient launch)."""
import pytest
import torch

from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import aux_grad_common as AG
from tests import parity_common as PC
from tests import plan_common as PL
from tests.emu_util import emu_library

pytestmark = pytest.mark.emu


def test_golden_reference_module():
    AG.check_golden(emu_library(), "cpu")


@pytest.mark.parametrize("shape", list(AG.SHAPES))
def test_module_dh_vs_oracle(shape):
    AG.check_module_dh(shape, emu_library(), "cpu")


def test_mol_head_dh():
    AG.check_mol_dh(emu_library(), "cpu")


ROWS = PL.pairwise_rows()
CASES = [(s, r) for s in ("P1", "P4") for r in ROWS]


@pytest.mark.parametrize("shape,row", CASES, ids=["%s-%s" % (s, PL.row_id(r)) for s, r in CASES])
def test_launch_plan_matrix_dh(shape, row):
    AG.check_row(shape, row, emu_library(), "cpu")


def _forward(shape, flags):
    params, x, h, t, ref = AG.instance(shape)
    eng = AG.engine_for(shape, emu_library(), "cpu", flags)
    _, dl = eng.forward_loss(x, h, t)
    return eng, dl, ref


@pytest.mark.parametrize("shape", ["P1", "P4", "N1"])
def test_dh_bits_do_not_depend_on_the_plan(shape):
    """dh is one fixed-order contraction of dP / dG: the same bits with and without the weight gradients, under every flush
    group size, bucket size and overlap mode (none of them changes dP), and on a second identical call."""
    eng, dl, ref = _forward(shape, DEFAULT_FLAGS)
    L = AG.SHAPES[shape][0][4] * AG.SHAPES[shape][0][5]
    base = AG.dh_call(eng, dl)
    assert bool(torch.isfinite(base).all()) and PC.rel_to_max(base, ref) <= PC.TOL_GRAD
    assert torch.equal(AG.dh_call(eng, dl), base), "two identical calls"
    assert torch.equal(AG.dh_call(eng, dl, grads=False), base), "grads == NULL"
    for n in (1, 2, L - 1):
        assert torch.equal(AG.dh_call(eng, dl, flags_extra=_lib.flag_dw_flush(n)), base), "DW_FLUSH(%d)" % n
    for lpb in (1, 2):
        assert torch.equal(AG.dh_call(eng, dl, lpb=lpb), base), "layers_per_bucket %d" % lpb
    for ov in (_lib.FLAG_BWD_OVERLAP, _lib.FLAG_BWD_OVERLAP | _lib.FLAG_BWD_OVERLAP_HEAD):
        assert torch.equal(AG.dh_call(eng, dl, flags_extra=ov), base), "overlap %#x" % ov
        assert torch.equal(AG.dh_call(eng, dl, flags_extra=ov, grads=False), base), "overlap %#x, grads == NULL" % ov


@pytest.mark.parametrize("flags,keep_scale", [(DEFAULT_FLAGS, True), (SIX_PRODUCT_FLAGS | _lib.FLAG_DW_F16PAIR, False),
                                              (SIX_PRODUCT_FLAGS, False)], ids=["default", "six_dw16", "six"])
@pytest.mark.parametrize("shape", ["P1", "P4", "N1"])
def test_frozen_call_launches_no_weight_gradient(shape, flags, keep_scale):
    """grads == NULL: no weight-gradient launch, no reduction of one, no bucket event, no scale of the fp16 pair weight
    gradients (DEFAULT_FLAGS keeps it: MM_F16PAIR's data contractions use it); a NaN-poisoned gradient buffer stays as it was."""
    eng, dl, ref = _forward(shape, flags)
    eng.grads().fill_(float("nan"))
    h = eng._last_inputs[1]
    dh = torch.full(h.shape, float("nan"))
    seq = PC.launch_sequence(eng.lib, lambda: eng.backward(dl, dh=dh, param_grads=False))
    assert "aux_dh" in seq, seq
    assert AG.weight_gradient_tags(seq, keep_scale) == [], seq
    assert bool(torch.isnan(eng.grads()).all())
    assert PC.rel_to_max(dh, ref) <= PC.TOL_GRAD


def test_loss_and_backward_default_issues_no_dh_launch():
    cfg, B, T = AG.SHAPES["P1"]
    params, x, h, t, ref = AG.instance("P1")
    model = WaveNet(*cfg, _library=emu_library())
    model.load_state_dict(params)
    seq = PC.launch_sequence(model.engine.lib, lambda: model.loss_and_backward(x, h, t))
    assert not [s for s in seq if s.startswith("aux_dh")], seq
    seq2 = PC.launch_sequence(model.engine.lib, lambda: model.loss_and_backward(x, h, t, aux_grad=True))
    # the same launches plus dh's own: the training step is unchanged around it
    assert [s for s in seq2 if not s.startswith("aux_dh")] == seq
    loss, dh = model.loss_and_backward(x, h, t, aux_grad=True)
    assert PC.rel_to_max(dh, ref) <= PC.TOL_GRAD


def test_frozen_model_autograd():
    """No parameter requires a gradient: autograd asks for dh alone (param_grads=False), the parameters get no .grad."""
    cfg, B, T = AG.SHAPES["P4"]
    params, x, h, t, ref = AG.instance("P4")
    model = WaveNet(*cfg, _library=emu_library())
    model.load_state_dict(params)
    model.requires_grad_(False)
    hv = h.detach().clone().requires_grad_(True)
    out = model(x, hv)
    rf = model.receptive_field
    loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, cfg[0]), t[:, rf:].contiguous().view(-1))
    loss.backward()
    assert PC.rel_to_max(hv.grad, ref) <= PC.TOL_GRAD
    assert all(p.grad is None for p in model.parameters())


def test_errors():
    eng, dl, ref = _forward("P1", DEFAULT_FLAGS)
    h = eng._last_inputs[1]
    rc, err = AG.call_backward_dh(eng, dl, None, None)
    assert rc != 0 and "NULL" in err, (rc, err)
    dh = torch.zeros(h.shape)
    rc, err = AG.call_backward_dh(eng, dl, None, dh, n_events=3)
    assert rc != 0 and "events" in err, (rc, err)
    rc, err = AG.call_backward_dh(eng, dl, None, dh)
    assert rc == 0 and err == "", (rc, err)
    rc, err = AG.call_backward_dh(eng, dl, eng.grads(), None)   # dh == NULL: wn_backward_window
    assert rc == 0, err
    with pytest.raises(ValueError):
        eng.backward(dl, dh=torch.zeros(h.shape[0], h.shape[1], h.shape[2] + 1))
    with pytest.raises(ValueError):
        eng.backward(dl, dh=torch.zeros(h.shape, dtype=torch.float64))
    with pytest.raises(ValueError):
        eng.backward(dl, dh=torch.zeros(h.shape[0], h.shape[2], h.shape[1]).transpose(1, 2))
    with pytest.raises(ValueError):
        eng.backward(dl, param_grads=False)
