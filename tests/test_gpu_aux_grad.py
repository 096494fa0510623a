# -*- coding: utf-8 -*-
"""MI355X: the gradient with respect to the aux features (dL/dh, wn_backward_dh) -- the emulator cases on the device, the
headline geometry with and without the upsampling layer against the oracle on the CPU, a frozen model, and an upstream
nn.Conv1d that produces h."""
import os

import pytest
import torch

from oracle import wavenet_oracle as O
from pytorchwavenetvocoder_amd import _lib
from pytorchwavenetvocoder_amd.engine import DEFAULT_FLAGS, SIX_PRODUCT_FLAGS
from pytorchwavenetvocoder_amd.nets import WaveNet
from tests import aux_grad_common as AG
from tests import parity_common as PC
from tests import plan_common as PL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_gpu():
    return _lib.load_library()


def test_golden_reference_module_gpu():
    AG.check_golden(_lib_gpu(), DEV)


@pytest.mark.parametrize("shape", list(AG.SHAPES))
def test_module_dh_vs_oracle_gpu(shape):
    AG.check_module_dh(shape, _lib_gpu(), DEV)


def test_mol_head_dh_gpu():
    AG.check_mol_dh(_lib_gpu(), DEV)


ROWS = PL.pairwise_rows()
CASES = [(s, r) for s in PL.SHAPES for r in ROWS]


@pytest.mark.parametrize("shape,row", CASES, ids=["%s-%s" % (s, PL.row_id(r)) for s, r in CASES])
def test_launch_plan_matrix_dh_gpu(shape, row):
    AG.check_row(shape, row, _lib_gpu(), DEV)


@pytest.mark.parametrize("shape", ["P1", "P4", "N1"])
def test_dh_bits_gpu(shape):
    """The same bits with and without the weight gradients, across flush / bucket / overlap knobs, and call to call."""
    params, x, h, t, ref = AG.instance(shape)
    eng = AG.engine_for(shape, _lib_gpu(), DEV, DEFAULT_FLAGS)
    _, dl = eng.forward_loss(x.cuda(), h.cuda(), t.cuda())
    base = AG.dh_call(eng, dl)
    assert bool(torch.isfinite(base).all()) and PC.rel_to_max(base, ref) <= PC.TOL_GRAD
    assert torch.equal(AG.dh_call(eng, dl), base)
    assert torch.equal(AG.dh_call(eng, dl, grads=False), base)
    for extra, lpb in ((_lib.flag_dw_flush(1), 0), (0, 1), (_lib.FLAG_BWD_OVERLAP, 0), (_lib.FLAG_BWD_OVERLAP | _lib.FLAG_BWD_OVERLAP_HEAD, 2)):
        assert torch.equal(AG.dh_call(eng, dl, flags_extra=extra, lpb=lpb), base), (extra, lpb)
        assert torch.equal(AG.dh_call(eng, dl, flags_extra=extra, lpb=lpb, grads=False), base), (extra, lpb)


def _threads():
    try:
        return max(1, min(16, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 4


@pytest.mark.parametrize("U", [80, 0])
def test_headline_geometry_vs_oracle(U):
    """(256, 80, 64, 256, 10, 3, 2, U) at T = 23040, B = 2 under DEFAULT_FLAGS and SIX_PRODUCT_FLAGS: ReLU kinks are certain at
    this size, so the oracle back-propagates with the HIP path's own ReLU masks (tests/parity_common.run_fullsize_vs_oracle)."""
    cfg_t = (256, 80, 64, 256, 10, 3, 2, U)
    B, T = 2, 23040
    cfg = O.OracleConfig(*cfg_t)
    params = O.random_params(cfg, 11, scale=0.05)
    x, h, t = O.synthetic_batch(cfg, B, T, 12)
    model = WaveNet(*cfg_t)
    model.load_state_dict(params)
    model.cuda()
    eng = model.engine
    for name, flags in (("default", DEFAULT_FLAGS), ("six", SIX_PRODUCT_FLAGS)):
        eng.flags = flags   # (each arithmetic's own forward: its own ReLU masks)
        loss, dh = model.loss_and_backward(x.cuda(), h.cuda(), t.cuda(), aux_grad=True)
        dh = dh.cpu()
        masks = ((eng.saved(_lib.WS_RELU_SKIP) > 0).float().cpu(), (eng.saved(_lib.WS_RELU_POST1) > 0).float().cpu())
        old = torch.get_num_threads()
        torch.set_num_threads(_threads())
        try:
            ref = AG.dh64(cfg_t, params, x, h, t, relu_masks=masks, dtype=torch.float32)
        finally:
            torch.set_num_threads(old)
        assert bool(torch.isfinite(dh).all()), name
        e = PC.rel_to_max(dh, ref)
        assert e <= PC.TOL_GRAD, (name, e)


def test_frozen_model_gpu():
    cfg, B, T = AG.SHAPES["P1"]
    params, x, h, t, ref = AG.instance("P1")
    model = WaveNet(*cfg)
    model.load_state_dict(params)
    model.cuda().requires_grad_(False)
    hv = h.detach().clone().cuda().requires_grad_(True)
    out = model(x.cuda(), hv)
    rf = model.receptive_field
    loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, cfg[0]), t.cuda()[:, rf:].contiguous().view(-1))
    loss.backward()
    assert PC.rel_to_max(hv.grad.cpu(), ref) <= PC.TOL_GRAD
    assert all(p.grad is None for p in model.parameters())


def test_upstream_conv_gets_its_gradient():
    """An nn.Conv1d on the GPU produces h: its weight gradient matches the same composition on the oracle (fp64)."""
    cfg_t, B, T = AG.SHAPES["P1"]
    params, x, h, t, _ = AG.instance("P1")
    cfg = O.OracleConfig(*cfg_t)
    torch.manual_seed(3)
    conv = torch.nn.Conv1d(cfg.n_aux, cfg.n_aux, 3, padding=1)
    w0, b0 = conv.weight.detach().clone(), conv.bias.detach().clone()
    model = WaveNet(*cfg_t)
    model.load_state_dict(params)
    model.cuda()
    conv.cuda()
    out = model(x.cuda(), conv(h.cuda()))
    rf = model.receptive_field
    loss = torch.nn.CrossEntropyLoss()(out[:, rf:].contiguous().view(-1, cfg.n_quantize), t.cuda()[:, rf:].contiguous().view(-1))
    loss.backward()
    w = w0.double().requires_grad_(True)
    b = b0.double().requires_grad_(True)
    p = {k: v.double() for k, v in params.items()}
    ref_loss = O.loss_fn(cfg, O.forward(cfg, p, x, torch.nn.functional.conv1d(h.double(), w, b, padding=1)), t)
    gw, gb = torch.autograd.grad(ref_loss, (w, b))
    assert abs(float(loss) - float(ref_loss)) <= PC.TOL_LOSS
    assert PC.rel_to_max(conv.weight.grad.cpu(), gw.float()) <= PC.TOL_GRAD
    assert PC.rel_to_max(conv.bias.grad.cpu(), gb.float()) <= PC.TOL_GRAD
